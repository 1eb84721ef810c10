"""``sggan`` -- host-side mirror of the reference's trainer object (model.py:39-566), hot path only.

``train_step`` follows model.py:169-200 line by line (documented deviations: D2 -- ``fake_A =
G(real_A)`` every step and ``da_fake`` evaluated once, since :187 and :188 are the same values).
Everything numeric runs in libsggan.so; this file sequences kernels, owns the flat
parameter/gradient buffers and (optionally) overlaps the data-parallel gradient all-reduce
(RCCL over xGMI; one bucket per network) with the remaining backward work.
"""
from __future__ import annotations

import contextlib
import math
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _abi as A
from . import evaluate as E
from . import kernels as K
from .graph import StepProgram
from .module import Adam, check_d_norm, check_upsample, Discriminator, DiscriminatorPair, Generator, GeneratorPair, GeneratorUNet, GeneratorUNetPair
from .utils import ImagePool, save_images, StaticImagePool

_DTYPES = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "f32": torch.float32, "fp32": torch.float32,
           "float32": torch.float32, torch.bfloat16: torch.bfloat16, torch.float32: torch.float32}


def default_args(**over):
    """The reference's argparse defaults (main.py:14-43) for the flags the step consumes, plus the
    build's own knobs (dtype/device/n_blocks/seed), as a namespace."""
    a = dict(batch_size=1, image_height=128, image_width=128, input_nc=3, output_nc=3, ngf=64, ndf=64,
             segment_class=34, beta1=0.5, lr=0.0002, L1_lambda=10.0, Lg_lambda=5.0, use_resnet=True, use_pix2pix=False,
             use_lsgan=True, ratio_gan2seg=10, max_size=50, phase="train", dataset_dir="city",
             dtype="bf16", device="cuda", n_blocks=9, seed=19, graph=False, mixed=False, paired=None,
             fuse_in_stats=True, fuse_in_bwd=False, g_buckets=3, keep_tapes=False, group2=True, d_quad=True,
             checkpoint_blocks=False, use_pool=False, pool_static=False, fuse_in_stats_deconv=False, fuse_in_stats_stem=False,
             crf=False, lr_decay=False, clip_grad_norm=0.0, skip_nonfinite=False, ema_decay=None, diffaug=None,
             diffaug_brightness=0.25, swd=False, swd_patches=128, ssim_lambda=0.0, ssim_data_range=1.0, d_norm="instance",
             dropout=None, upsample="deconv", fm_lambda=0.0)
    a.update(over)
    return SimpleNamespace(**a)


def _spectral_state(net):
    """The network's power-iteration vectors, or None for a network without spectral norm (any object with a ``P``)."""
    f = getattr(net, "spectral_state", None)
    return None if f is None else f()


class sggan(object):
    # model.py:151 ``LAMBDA = 100`` (hard-coded; --L1_lambda is ignored by the live step) and
    # model.py:205 ``lr = 0.001`` (hard-coded; --lr is ignored) -- SURVEY.md 5 "Config / flags".
    LAMBDA = 100.0
    LR = 0.001
    _swd_add_reals = staticmethod(E.swd_add_reals)      # (the name the SWD tests call it by)

    def __init__(self, args=None, **kw):
        args = args if args is not None else default_args(**kw)
        g = lambda k, d=None: getattr(args, k, d)
        self.batch_size = g("batch_size", 1)
        self.image_width, self.image_height = g("image_width", 128), g("image_height", 128)
        self.input_c_dim, self.output_c_dim = g("input_nc", 3), g("output_nc", 3)
        self.segment_class = g("segment_class", 34)
        self.use_pix2pix = bool(g("use_pix2pix", False))
        if self.use_pix2pix:
            raise NotImplementedError("use_pix2pix: generator_pix2pix / discriminator_pix2pix (BatchNorm, 4x4 stride-2 U-Net) are "
                                      "not built (SURVEY.md 2.1); use_pix2pix=False selects the mask discriminator")
        # model.py:55-62: --use_resnet picks generator_resnet(), otherwise generator_unet() (the reference's flag-less default)
        self.arch = "resnet" if g("use_resnet", True) else "unet"
        self.cycle = bool(g("cycle", False))
        # dropout (off by default -- the reference's own calls run the generator in inference mode): the rate of
        # generator_unet's three Dropout layers (d1..d3, module.py:170-180).  Given, the train step runs the generators in training
        # mode: each site masks its conv output in place, forward and backward, with a mask regenerated from the generator's own
        # seed and device step counter, the application (0: the pass over a real batch, 1: the pass over the other generator's
        # fakes), the layer and the global sample index -- no new state, so graph replay, checkpoints and data parallelism see the
        # masks of the plain single-device run.  Every other caller (the test passes, generator(x)) stays in inference mode.
        drop = g("dropout", None)
        self.dropout = None if drop is None else float(drop)
        if self.dropout is not None:
            if not 0.0 <= self.dropout < 1.0:
                raise ValueError(f"dropout must lie in [0, 1), got {drop!r}")
            if self.arch == "resnet":
                raise ValueError("--dropout: generator_resnet has no dropout layers (the reference's are in generator_unet: "
                                 "--generator unet / use_resnet=False)")
        # d_norm ("instance" is the reference's network): "spectral" builds the discriminators without instance
        # norms and runs every one of their convs on W / sigma(W) -- one power iteration per discriminator per training step
        # (Discriminator.spectral_step, first thing in the step bodies), the gradient transform directly before their Adam
        # launch (_apply_gradients).  The whole state is one small vector per layer on the device, advanced by the step's own
        # launches: graph replay and checkpoints carry it, and data-parallel ranks, which hold identical W and u (rank 0's:
        # enable_data_parallel), compute identical sigma without exchanging anything.  The generators never see it.
        self.d_norm = check_d_norm(g("d_norm", "instance"))
        # upsample ("deconv" is the reference's network): "nearest" / "bilinear" build generator_resnet's two
        # doubling layers as a fixed 2x resampling + a 3x3 stride-1 SAME conv (Odena et al. 2016) -- same parameter names and
        # sizes, d1_w / d2_w in the Conv2D layout.  The resampling has no parameters and no state: every other option, graph
        # replay, checkpoints and data parallelism see an ordinary conv unit with one launch in front and one behind.
        self.upsample = check_upsample(g("upsample", "deconv") or "deconv")
        if self.upsample != "deconv" and self.arch != "resnet":
            raise ValueError("--upsample: generator_unet has no stride-2 layer to replace (all of its convs are stride 1: the option "
                             "belongs to generator_resnet's d1 / d2: --generator resnet / use_resnet=True)")
        # fm_lambda (off by default): the paired step's generator loss also gets fm_lambda * the feature-matching
        # term of pix2pixHD -- the mean over D's seven intermediate activations of mean |D_k(fake) - D_k(seg)| -- from ONE
        # K.feature_match call on the tape D's pass already recorded; its seven gradients join the generator-gradient walk through D
        # in the data-gradient stores (feature_addends).  D's own gradient never sees the term, and it keeps no state: graph
        # replay, checkpoints and data parallelism (a per-rank mean, averaged like L1) need nothing.  0: no launch, no buffer.
        fm = g("fm_lambda", 0.0)
        self.fm_lambda = float(fm or 0.0)
        if not (math.isfinite(self.fm_lambda) and self.fm_lambda >= 0.0):
            raise ValueError(f"fm_lambda must be finite and >= 0, got {fm!r}")
        if self.fm_lambda and self.cycle:
            raise ValueError("--fm_lambda with --cycle: the cycle step's fakes have no pixel-aligned real, so there is no per-sample "
                             "feature target; the term belongs to the paired (reference-mode) step")
        if self.fm_lambda and K.diffaug_policy_bits(g("diffaug", None)):
            raise ValueError("--fm_lambda with --diffaug: reals and fakes take independent draws, so their discriminator features "
                             "stop corresponding; train with one of the two")
        self.dtype = _DTYPES[g("dtype", "bf16")]
        self.device = torch.device(g("device", "cuda"))
        if self.device.type != "cuda":       # refused here, before any network (and so any buffer) is built
            raise NotImplementedError(f"sggan(cycle={self.cycle}, generator={self.arch}) on device '{self.device}': the train step has "
                                      "no host implementation, it runs on the MI355X HIP path only (device must be a cuda/hip device)")
        seed = g("seed", 19)
        self.discriminator = Discriminator(df_dim=g("ndf", 64), in_c=self.output_c_dim, segment_class=self.segment_class,
                                           dtype=self.dtype, device=self.device, seed=seed + 1, norm=self.d_norm)   # model.py:54
        def make_generator(in_c, out_c, seed):                  # :56 generator_resnet / :58 generator_unet
            kw = dict(gf_dim=g("ngf", 64), in_c=in_c, out_c=out_c, dtype=self.dtype, device=self.device, seed=seed)
            if self.arch == "resnet":
                return Generator(n_blocks=g("n_blocks", 9), upsample=self.upsample, **kw)
            return GeneratorUNet(**kw) if self.dropout is None else GeneratorUNet(dropout=self.dropout, **kw)
        self.generator = make_generator(self.input_c_dim, self.output_c_dim, seed)
        self.beta1 = g("beta1", 0.5)
        self.lr = self.LR
        # cycle mode (north_star unit, deviation D5): G_A->B = self.generator, D_A = self.discriminator, plus G_B->A and D_B
        self.L1_lambda, self.Lg_lambda = float(g("L1_lambda", 10.0)), float(g("Lg_lambda", 5.0))
        self.use_lsgan = bool(g("use_lsgan", True))
        self.cycle_lr = float(g("lr", 0.0002))
        if self.cycle:
            self.generator_BA = make_generator(self.output_c_dim, self.input_c_dim, seed + 2)
            self.discriminator_B = Discriminator(df_dim=g("ndf", 64), in_c=self.output_c_dim, segment_class=self.segment_class,
                                                 dtype=self.dtype, device=self.device, seed=seed + 3, norm=self.d_norm)
            self.real_B = self.seg_B = self.mask_B = self.fake_B = None
        # step I/O attributes (model.py:250-256 sets the inputs; :260 reads the losses)
        self.real_A = self.seg_A = self.mask_A = self.fake_A = None
        self._loss = torch.zeros(2, dtype=torch.float32, device=self.device)    # [gen_loss, disc_loss] on device
        self.gen_loss, self.disc_loss = self._loss[0:1], self._loss[1:2]
        self.fm_loss = torch.zeros(1, dtype=torch.float32, device=self.device) if self.fm_lambda else None   # the term itself
        self._dp = None
        self._world = 1
        self.dataset_dir = g("dataset_dir", "city")
        # model.py:79 builds ImagePool(args.max_size) but the fork never calls it; it is used by the cycle step when
        # use_pool is set (upstream SG-GAN behaviour: D sees a history of fakes)
        self.use_pool = bool(g("use_pool", False))
        # pool_static: the pool step with a fixed launch sequence (utils.StaticImagePool: decisions on the host, selects on the
        # device) -- what graph replay needs; the dynamic form (D judges the pooled fakes in their own pass only when the pool
        # hands back older ones) stays the default of the eager path
        self.pool_static = bool(g("pool_static", False)) or (self.use_pool and bool(g("graph", False)))
        self.pool = (StaticImagePool if self.pool_static else ImagePool)(g("max_size", 50), rng=g("pool_rng", None))
        # diffaug (off by default): every image a discriminator sees -- reals and fakes -- goes through ONE random,
        # differentiable transform first (Zhao et al. 2020: colour and cutout; translation is left out, the mask D multiplies
        # into its last map cannot follow a pixel shift).  D reads an augmented COPY of its stacked input, the generators' loss
        # backpropagates through the transform's adjoint, which also takes over the gradient join (``addend``).  The rows of
        # parameters are drawn on the device from D's own step counter and the global sample index (K.diffaug_draw), so there is
        # no new state: graph replay, checkpoints and data parallelism see the draws of the plain single-device run.
        self.diffaug = K.diffaug_policy_bits(g("diffaug", None))
        self.diffaug_brightness = float(g("diffaug_brightness", 0.25))
        # (_diffaug_bits: the policy bits handed to the draw launches, apart from ``diffaug``, which gates the wiring, for ONE reason:
        # the wiring test sets it to 0 on a built model, so that the option's own launches write neutral rows.  Nothing else writes it.)
        self._diffaug_bits, self._diffaug_seed = self.diffaug, int(seed)
        if self.diffaug and self.use_pool:
            raise NotImplementedError("diffaug with use_pool: the draws are keyed by (discriminator step, global sample index), and a "
                                      "fake handed back by the image pool carries no sample identity (nor the step it was made at); "
                                      "train with one of the two")
        # ssim_lambda (off by default): beside every L1 reconstruction term the generators' loss gets
        # ssim_lambda * (1 - mean SSIM(target, reconstruction)) -- K.ssim_loss, one call after each K.l1_loss, into the same loss
        # cell and the same gradient buffer.  The term never sees a discriminator and keeps no state: graph replay, the image
        # pool, diffaug and data parallelism (a per-rank mean, averaged like L1) need nothing.  0: no launch, no buffer.
        self.ssim_lambda = float(g("ssim_lambda", 0.0) or 0.0)
        self.ssim_data_range = float(g("ssim_data_range", 1.0))
        if not (math.isfinite(self.ssim_lambda) and self.ssim_lambda >= 0.0):
            raise ValueError(f"ssim_lambda must be finite and >= 0, got {g('ssim_lambda')!r}")
        if self.ssim_lambda and not (math.isfinite(self.ssim_data_range) and self.ssim_data_range > 0.0):
            raise ValueError(f"ssim_data_range must be finite and > 0, got {g('ssim_data_range')!r}")
        if self.ssim_lambda and min(self.image_height, self.image_width) < 11:
            raise ValueError(f"--ssim_lambda: SSIM's 11x11 window needs training images of at least 11x11 pixels, "
                             f"got {self.image_height}x{self.image_width}")
        self.pair_wgrads = bool(g("pair_wgrads", True))   # cycle step: one weight-gradient launch per layer for both applications of a G
        self.batch_d_real_fake = bool(g("batch_d_real_fake", True))   # pool mode: D(real) and D(pooled fakes) as one 2N pass
        self.d_quad = bool(g("d_quad", True))             # reals and fakes through the discriminator(s) as ONE stacked pass (both step flavours)
        self.gen_loss_metric, self.disc_loss_metric, self._metric_n = 0.0, 0.0, 0
        # model.py:83-84 / 205-207: one Keras Adam per network (lr hard-coded 1e-3 on the live step; the cycle step
        # uses --lr).  d_optim / g_optim are the reference's attribute names; the cycle step adds the other two.
        lr = self.cycle_lr if self.cycle else self.lr
        # lr_decay: the linear decay of model.py:223 (commented out there), evaluated on the device by every optimizer's update
        # from its own step counter and ONE descriptor [steps_per_epoch, epoch_step, epochs] all of them share.  It exists
        # from here on and starts as "never decays", so a step recorded before train() carries its address;
        # set_lr_schedule only writes into it.  Each optimizer's learning_rate is the base rate.
        self.lr_decay = bool(g("lr_decay", False))
        self._lr_sched = torch.tensor([1, 0, 0], dtype=torch.int64, device=self.device) if self.lr_decay else None
        self._lr_sched_host = (1, 0, 0)
        # clip_grad_norm / skip_nonfinite (no counterpart in the reference, off by default): every optimizer
        # measures its network's global gradient norm on the device, clips to clip_grad_norm (> 0) and skips an update whose
        # gradient is not finite -- decided by the update's own launches, so it costs no host sync and survives graph replay
        self.clip_grad_norm = max(float(g("clip_grad_norm", 0.0) or 0.0), 0.0)
        self.skip_nonfinite = bool(g("skip_nonfinite", False))
        okw = dict(schedule=self._lr_sched, clip_norm=self.clip_grad_norm or None, skip_nonfinite=self.skip_nonfinite)
        # ema_decay (off by default): the generators' updates also keep an exponential moving average of their
        # parameters, in the update's own launches -- the decay ramp follows the device step counter and a skipped update
        # leaves the average alone -- and the test passes run on the average (ema_weights).  Data parallel: nothing to
        # exchange per step, every rank applies the same update to the same average -- the same because enable_data_parallel
        # broadcasts rank 0's average with the rest of the replicated state.
        ema = g("ema_decay", None)
        self.ema_decay = None if ema is None else float(ema)
        if self.ema_decay is not None and not 0.0 < self.ema_decay < 1.0:
            raise ValueError(f"ema_decay must lie in (0, 1), got {ema!r}")
        gkw = dict(okw, ema_decay=self.ema_decay)
        self.g_optim = Adam(self.generator, lr, self.beta1, **gkw)
        self.d_optim = Adam(self.discriminator, lr, self.beta1, **okw)
        if self.cycle:
            self.g_optim_BA = Adam(self.generator_BA, lr, self.beta1, **gkw)
            self.d_optim_B = Adam(self.discriminator_B, lr, self.beta1, **okw)
        if self.ema_decay is not None:
            for net in self._ema_nets():
                net.P.enable_ema()
        self._ema_notice = self._sn_notice = False
        # cycle step: run the two generators (and the two discriminators) in lockstep on stacked batches (module._PairUnit);
        # bit-identical to the one-network-at-a-time sequencing, which stays for the image pool and for mixed mode.  paired=None
        # picks the default: on for the ResNet (the step bench.py times); off for the U-Net, whose step is bound by
        # full-resolution 512-channel halo GEMMs that pairing does not touch -- lockstep is 4 % faster at 128x128 batch 8 but
        # 0.6 % slower (and 8 GB larger) at 256x512 batch 8, more than the run-to-run spread ("cycle mode")
        paired = g("paired", None)
        self.paired = bool(paired) if paired is not None else self.arch == "resnet"
        # mixed precision: bf16 storage, but the activation-gradient chain through the generators' residual blocks in f32
        self.mixed = bool(g("mixed", False)) and self.dtype == torch.bfloat16
        for net in self.networks():
            net.mixed = self.mixed
            # conv epilogue -> norm statistics (on), data-gradient epilogue -> norm-backward sums (opt-in; module.py)
            net.fuse_in_stats, net.fuse_in_bwd = bool(g("fuse_in_stats", True)), bool(g("fuse_in_bwd", False))
            net.fuse_in_stats_deconv, net.fuse_in_stats_stem = bool(g("fuse_in_stats_deconv", False)), bool(g("fuse_in_stats_stem", False))
            net.group2 = bool(g("group2", True))
            # activation checkpointing (BASELINE.json configs[4]): the generators keep each residual block's input only and
            # re-run the block (module.py:208-217) in backward -- bitwise the same gradients, + 2 conv forwards per block
            net.checkpoint_blocks = bool(g("checkpoint_blocks", False)) and isinstance(net, Generator)
        # data parallel: each generator's gradient buffer is exchanged as this many contiguous layer-group buckets, launched
        # in backward-completion order so that all but the last overlap the rest of the backward pass
        self.g_buckets = max(1, int(g("g_buckets", 3)))
        # diagnostics: keep the last step's forward records (saved activations) reachable as ``self.tapes`` -- the parity tests
        # read from them which side of each ReLU / LeakyReLU kink the kernels took (tests/kink_helpers.py).  Off: they are dropped
        # when the step returns, so their memory is reused at once.
        self.keep_tapes = bool(g("keep_tapes", False))
        self.tapes = None
        # HIP-graph replay of the step (graph.py): recorded at the first train_step after enable_graph()
        self.use_graph = bool(g("graph", False))
        self._program = None
        self._static_in = {}
        self._stack_bufs = {}                       # persistent stacked-batch buffers of the step (_stacked)

    # ------------------------------------------------------------------ data parallel (new capability)
    def enable_data_parallel(self, process_group=None):
        """Average gradients over ranks with one all-reduce per network, launched as soon as that
        network's backward has been queued so it overlaps with the rest of the step (dp.GradExchange).

        Every claim the options make about data parallelism ("ranks hold identical W and u", "every rank applies the same update
        to the same average", "the draws of the single-device run") rests on the replicas being identical, and this call is what
        makes them so: every rank takes rank 0's replicated state -- all that ``state_dict`` writes: parameters, Adam slots and step
        counter, the guard's counters, the weight average, the spectral u -- and rank 0's draw keys (the networks' seeds, which
        key the dropout masks and the seeded start of u, and the augmentation's seed).  However the ranks were built, seeded or
        resumed, they leave this call equal bit for bit; what a rank draws then differs by its sample offset alone."""
        from .dp import GradExchange
        self._dp = GradExchange(process_group)
        self._world = self._dp.world
        nets = self.networks()
        # host side first: the draw keys, and which networks carry a guard record on rank 0 (a checkpoint's counters allocate it
        # at load, a fresh model at its first guarded step), so that every rank enters the same collectives below
        keys = self._dp.broadcast_object({"seeds": [n.seed for n in nets], "diffaug": self._diffaug_seed,
                                          "guard": [n.P._guard is not None for n in nets]})
        self._diffaug_seed = int(keys["diffaug"])
        for net, seed, guard in zip(nets, keys["seeds"], keys["guard"]):
            P = net.P
            net.adopt_seed(seed)
            state = [P.flat, P.m, P.v, P._adam_state]
            if guard:
                state.append(P.guard_buffers()[0])
            elif P._guard is not None:                          # (rank 0 has counted nothing)
                P._guard.zero_()
            if P.ema is not None:
                state += [P.ema, P._ema_state]
            u = _spectral_state(net)
            if u is not None:
                state.append(u)
            for t in state:
                self._dp.broadcast_(t)
            P.version += 1
            if u is not None and self._world > 1:               # u may have been replaced: sigma is computed anew
                net._sn.seen = None
        self._program = None                                    # a recorded step has no collectives in it: record again
        return self

    def _host(self, fn):
        """A host-side action at this point of the step (graph.StepProgram.host): called right away on the eager
        path; while the step is being recorded it ends the current HIP-graph segment and is replayed between segments."""
        return K.host(fn)

    def _allreduce(self, net, lo=None, hi=None, handle=None):
        """Launch the all-reduce of one network's gradient bucket (the whole flat buffer, or its [lo, hi) range); the
        returned handle's wait() orders the stream behind every bucket launched on it."""
        if self._dp is None:
            return None
        h = handle if handle is not None else _PendingReduce(self)
        buf = net.P.grad if lo is None else net.P.grad[lo:hi]
        def launch():
            h.works.append(self._dp.allreduce_async(buf))
        self._host(launch)
        return h

    def _bucketed_allreduce(self, nets):
        """(on_unit_done, handles) for the LAST backward pass of the generator(s) ``nets`` this step: each network's flat
        gradient buffer is cut into ``g_buckets`` contiguous layer groups (module.bucket_plan); a group's all-reduce is launched
        as soon as the backward of its first layer -- weight gradient included -- has been queued, i.e. while the layers in front
        of it are still being differentiated.  Networks that run in lockstep (the paired cycle step) share the host action."""
        if self._dp is None:
            return None, [None] * len(nets)
        plans = [{first: (lo, hi) for first, lo, hi in net.bucket_plan(self.g_buckets)} for net in nets]
        handles = [_PendingReduce(self) for _ in nets]

        def on_unit_done(name):
            ready = [(net, h, plan[name]) for net, h, plan in zip(nets, handles, plans) if name in plan]
            if not ready:
                return
            # a bucket may only travel once every weight gradient inside its range has been launched: a deferred (paired)
            # weight gradient that ran after its range's all-reduce would make the ranks diverge silently
            for net, _, (lo, hi) in ready:
                pend = [u for u in net.pending_wgrads() if lo <= net.P.index[u + "_w"][0] < hi]
                assert not pend, f"bucket [{lo}, {hi}) launched at {name} with weight gradients still deferred: {pend}"
            bufs = [(h, net.P.grad[lo:hi]) for net, h, (lo, hi) in ready]
            def launch():
                for h, buf in bufs:
                    h.works.append(self._dp.allreduce_async(buf))
            self._host(launch)
        return on_unit_done, handles

    # ------------------------------------------------------------------ HIP-graph replay (graph.py)
    def enable_graph(self, flag=True):
        """Replay the step from captured HIP graphs instead of dispatching ~1 250 launches from Python each step."""
        self.use_graph = bool(flag)
        if not flag:
            self._program = None
        return self

    _INPUTS_REF = ("real_A", "seg_A", "mask_A")
    _INPUTS_CYCLE = ("real_A", "seg_A", "mask_A", "real_B", "seg_B", "mask_B")

    def _convert_input(self, name, x):
        if name.startswith("mask"):
            m = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float32))
            return m.to(device=self.device, dtype=torch.float32).contiguous()
        return self._prep(x)

    def _stage_inputs(self):
        """Step inputs -> the static device buffers the recorded graphs read.  A buffer the caller fills in place (it is
        what ``self.real_A`` etc. point at after the first graph step) costs nothing; anything else is converted and copied."""
        names = self._INPUTS_CYCLE if self.cycle else self._INPUTS_REF
        fresh = False
        for n in names:
            x = getattr(self, n)
            buf = self._static_in.get(n)
            if buf is not None and x is buf:
                continue
            t = self._convert_input(n, x)
            if buf is None or buf.shape != t.shape or buf.dtype != t.dtype:
                self._static_in[n] = t.clone()
                fresh = True
            else:
                buf.copy_(t)
            setattr(self, n, self._static_in[n])
        return fresh

    def adopt_inputs(self, **buffers):
        """Make caller-owned device tensors the recorded step's static inputs (``real_A=..., seg_A=..., mask_A=...``): a
        loader that refills them in place (data.DirectoryBatches) then feeds a replayed step with no staging copy.  Images
        must already be in the internal layout (channel-padded, network dtype), masks float32."""
        names = self._INPUTS_CYCLE if self.cycle else self._INPUTS_REF
        for n, t in buffers.items():
            if n not in names:
                raise KeyError(f"{n}: not an input of this step ({', '.join(names)})")
            want = torch.float32 if n.startswith("mask") else self.dtype
            if not (isinstance(t, torch.Tensor) and t.device.type == self.device.type and t.is_contiguous() and t.dtype == want
                    and (n.startswith("mask") or t.shape[-1] % A.CPAD == 0)):
                raise ValueError(f"{n}: a contiguous {want} device tensor in the step's internal layout is required")
            self._static_in[n] = t
        self._program = None
        return self

    def _graph_step(self):
        if self.use_pool and not self.pool_static:
            raise NotImplementedError("graph replay with the dynamic image pool: its random swaps change the step's launch "
                                      "sequence; build the model with pool_static=True (or graph=True) or run the pool step eagerly")
        if self._stage_inputs():
            self._program = None                   # new shapes: record again
        if self._program is None:
            self._record()
        if self.use_pool:
            self.pool.stage(self.device)           # this step's pool decisions -> the device tensor the recorded selects read
        self._program.replay()
        for n in self.networks():
            n.P.version += 1                       # the replayed Adam changed the parameters: eager callers must re-pack
        return self.gen_loss, self.disc_loss

    def _record(self):
        """Warm up eagerly (kernel attributes, workspaces, weight-pack tables), put the parameters and optimizer state
        back, then record ONE step without executing it."""
        nets = self.networks()
        keep = [(n.P.flat.clone(), n.P.m.clone(), n.P.v.clone(), n.P.iterations.clone()) for n in nets]
        guard_keep = [None if n.P._guard is None else n.P._guard.clone() for n in nets]     # (the warm-up step counts as none)
        ema_keep = [None if n.P.ema is None else (n.P.ema.clone(), n.P._ema_state.clone()) for n in nets]
        sn_keep = [None if n.spectral_state() is None else n.spectral_state().clone() for n in nets]    # (the warm-up step's power iteration too)
        loss_keep = self._loss.clone()
        hook, K.PROFILE = K.PROFILE, None          # timing hooks (bench.py) record events: not while recording
        try:
            if self.use_pool:                      # the warm-up step: "return the input, store nothing" (no decision is consumed)
                cur = max(self.pool.maxsize, 0)
                if self.pool.ctrl is None:
                    self.pool.ctrl = torch.zeros(4, dtype=torch.int64, device=self.device)
                self.pool.ctrl.fill_(cur)
            self._step_body()
            torch.cuda.synchronize(self.device)
            for n, (f, m, v, it) in zip(nets, keep):
                n.P.flat.copy_(f); n.P.m.copy_(m); n.P.v.copy_(v); n.P.iterations.copy_(it)
                n.P.version += 1                   # the recorded step starts by re-packing the conv weights
            for n, rec in zip(nets, guard_keep):
                if n.P._guard is not None and rec is not None:
                    n.P._guard.copy_(rec)
                elif n.P._guard is not None:       # first allocated by the warm-up step
                    n.P._guard.zero_()
            for n, kept in zip(nets, ema_keep):
                if kept is not None:
                    n.P.ema.copy_(kept[0]); n.P._ema_state.copy_(kept[1])
            for n, u in zip(nets, sn_keep):
                if u is not None:
                    n.spectral_state().copy_(u)
            self._loss.copy_(loss_keep)
            prog = StepProgram(self.device)
            K._RECORDER = prog
            try:
                prog.record(self._step_body)
            finally:
                K._RECORDER = None
            # addresses baked into the recorded launches that do not come from the capture pool: the shared scratch workspace
            # and the networks' scratch vectors (allocated by the eager warm-up).  The program keeps them alive, so a later,
            # larger workspace request elsewhere in the process cannot hand their memory to another tensor under a replay.
            prog.keep = K.workspace_refs() + [n._scratch for n in nets if n._scratch is not None]
            self._program = prog
        finally:
            K.PROFILE = hook

    # ------------------------------------------------------------------ the hot path
    def _prep(self, x, out=None):
        t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float32))
        return self.generator.to_internal(t.to(self.device), out=out)

    def _stacked(self, key, shape, dtype):
        """A persistent device buffer for one of the step's stacked batches ([real_A; real_B], the discriminators' stacked input
        and masks): inputs are converted straight into its slices and the generators' last layer writes the fakes into it, so
        the step concatenates nothing."""
        bufs = self._stack_bufs
        buf = bufs.get(key)
        if buf is None or tuple(buf.shape) != tuple(shape) or buf.dtype != dtype:
            buf = bufs[key] = torch.empty(tuple(shape), dtype=dtype, device=self.device)
        return buf

    def _drop(self, application, n):
        """The keywords that put a U-Net generator's forward into training mode for this application (0: over a real batch, 1:
        over the other generator's fakes) of a batch of n per rank -- its samples are the global samples rank * n .., exactly
        as _diffaug_table counts them.  Without the option: none, the forward's launches are the inference ones."""
        if self.dropout is None:
            return {}
        return {"dropout": application, "sample_offset": (self._dp.rank if self._dp is not None else 0) * n}

    def _diffaug_table(self, n, H, W, streams):
        """The step's parameter table, n rows per entry of ``streams`` = ((discriminator, which_D, role), ...) in the row order of
        the batch it augments; role 0: reals, 1: fakes.  One draw launch per entry: each reads ITS discriminator's device step
        counter when it runs, and is keyed by the global sample index (rank * n + row), not by the row of the stacked buffer."""
        par = self._stacked("da_par", (len(streams) * n, 8), torch.float32)
        off = (self._dp.rank if self._dp is not None else 0) * n
        for i, (Dn, which, role) in enumerate(streams):
            K.diffaug_draw(par[i * n:(i + 1) * n], Dn.P.iterations, self._diffaug_seed, off, 2 * which + role, H, W, self._diffaug_bits,
                           self.diffaug_brightness)
        return par

    @property
    def diffaug_params(self):
        """The last step's parameter table (rows x 8, f32, on the device), in the row order of the discriminators' stacked input:
        reference step [real; fake], cycle step [D_B real; D_B fake; D_A fake; D_A real].  None before the first step."""
        return self._stack_bufs.get("da_par")

    def train_step(self, args=None):
        """model.py:169-200.  Reads ``real_A, seg_A`` (N,H,W,3) in [0,1] and ``mask_A`` (N,mh,mw,C);
        writes ``fake_A, gen_loss, disc_loss``; updates G, D and both Adam states."""
        if self.ssim_lambda and self.real_A is not None and min(self.real_A.shape[1:3]) < 11:     # (not the kernel's status mid-step)
            raise ValueError(f"--ssim_lambda: SSIM's 11x11 window needs training images of at least 11x11 pixels, "
                             f"got {self.real_A.shape[1]}x{self.real_A.shape[2]}")
        if self.use_graph:
            return self._graph_step()
        if self.use_pool and self.pool_static:
            self.pool.stage(self.device)
        return self._step_body()

    def _ssim_term(self, target, x, C, gl, dx):
        """ssim_lambda * (1 - mean SSIM(target, x)) added to ``gl``, its gradient w.r.t. x added to ``dx`` (which the L1 term
        in front of it has written).  Off: nothing is launched."""
        if self.ssim_lambda:
            K.ssim_loss(target, x, C, gl, dx, weight=self.ssim_lambda, data_range=self.ssim_data_range,
                        accumulate_loss=True, accumulate_grad=True)

    def _step_body(self):
        if self.cycle:
            return self._train_step_cycle()
        G, D = self.generator, self.discriminator
        D.spectral_step()           # (d_norm="spectral": this step's sigma, before D's first use; else nothing)
        # :186-188.  d_quad: D sees [seg; fake] as ONE stacked pass (half the launches; its tail layers are launch-latency bound);
        # the generator's loss backpropagates through the fake slice of the same tape.  Per image the same arithmetic.  The
        # stacked input is one persistent buffer: seg is converted into its first half, G writes the fakes into the second.
        stack = self.d_quad
        real = self._prep(self.real_A)
        N = real.shape[0]
        mask = self._convert_input("mask_A", self.mask_A)
        if stack:
            d_in = self._stacked("d_in", (2 * N,) + tuple(real.shape[1:]), real.dtype)
            seg = self._prep(self.seg_A, out=d_in[:N])
            mask2 = torch.cat([mask, mask], out=self._stacked("d_mask", (2 * N,) + tuple(mask.shape[1:]), mask.dtype))
        else:
            seg = self._prep(self.seg_A)
        G.P.zero_grad()
        D.P.zero_grad()

        fake, tG = G.forward(real, out=d_in[N:] if stack else None, **self._drop(0, N))   # :175-179 (D2)
        aug = bool(self.diffaug)
        d_seg, d_fake = seg, fake
        if aug:         # D judges augmented copies; ``seg`` and ``fake`` themselves stay as the L1 term reads them
            par = self._diffaug_table(N, real.shape[1], real.shape[2], ((D, 0, 0), (D, 0, 1)))
            d_aug = self._stacked("d_aug", (2 * N,) + tuple(real.shape[1:]), real.dtype)
            if stack:
                K.diffaug(d_in, par, self.output_c_dim, out=d_aug)
            else:
                d_seg = K.diffaug(seg, par[:N], self.output_c_dim, out=d_aug[:N])
                d_fake = K.diffaug(fake, par[N:], self.output_c_dim, out=d_aug[N:])
        if stack:
            da_both, tDq = D.forward(d_aug if aug else d_in, mask2)
            da_real, da_fake = da_both[:N], da_both[N:]
            tDr, tDf = None, D.slice_tape(tDq, N, 2 * N)
        else:
            da_real, tDr = D.forward(d_seg, mask)                           # :186
            da_fake, tDf = D.forward(d_fake, mask)                          # :187 (= :188)

        # losses + their logit gradients, all on device (no host sync)
        gl, dl = self._loss[0:1], self._loss[1:2]
        d_fake_g = torch.empty_like(da_fake)
        d_both_d = torch.empty((2 * N,) + tuple(da_real.shape[1:]), dtype=da_real.dtype, device=da_real.device)
        d_real_d, d_fake_d = d_both_d[:N], d_both_d[N:]
        dfake_l1 = torch.empty_like(fake)
        K.bce_logits(da_fake, 1.0, gl, d_fake_g)                            # :153 gan_loss
        K.l1_loss(seg, fake, self.output_c_dim, gl, dfake_l1, weight=self.LAMBDA, accumulate=True)   # :155-156
        self._ssim_term(seg, fake, self.output_c_dim, gl, dfake_l1)
        K.bce_logits(da_real, 1.0, dl, d_real_d)                            # :162
        K.bce_logits(da_fake, 0.0, dl, d_fake_d, accumulate_loss=True)      # :163-164 (adds to disc_loss)

        # disc_tape.gradient(disc_loss, D vars)  (:197)
        if stack:
            D.backward(tDq, d_both_d, want_dx=False, param_grads=True)
        else:
            D.backward(tDr, d_real_d, want_dx=False, param_grads=True)
            D.backward(tDf, d_fake_d, want_dx=False, param_grads=True)
        hD = self._allreduce(D)
        fm_grads = None
        if self.fm_lambda:      # + fm_lambda * mean_k mean |D_k(fake) - D_k(seg)|: the generator's loss only, the reals constants
            f_real, f_fake = (D.features(tDq, 0, N), D.features(tDq, N, 2 * N)) if stack else (D.features(tDr), D.features(tDf))
            fm_grads = K.feature_match(f_real, f_fake, [u.cout for u in D.units], gl, self.fm_loss, self.fm_lambda, accumulate_loss=True)
        # gen_tape.gradient(gen_loss, G vars)    (:196): through D's data path, then G
        if aug:         # ... and back through the transform's adjoint, which takes over the join
            dfake = K.diffaug_bwd(D.backward(tDf, d_fake_g, want_dx=True, param_grads=False), par[N:], self.output_c_dim, addend=dfake_l1)
        else:
            dfake = D.backward(tDf, d_fake_g, want_dx=True, param_grads=False, addend=dfake_l1,    # (the join rides on h0's data-gradient store,
                               feature_addends=fm_grads)                                          #  the feature gradients on h1's .. h4's)
        hook, (hG,) = self._bucketed_allreduce((G,))
        G.backward(tG, dfake, want_dx=False, param_grads=True, on_unit_done=hook)

        self._apply_gradients((self.d_optim, hD), (self.g_optim, hG))       # :200, :199
        self._fake_internal = fake
        self.fake_A = _LazyUnpad(fake, self.output_c_dim)
        self.da_real, self.da_fake = da_real, da_fake
        if self.keep_tapes:            # (stacked pass: views of its records, images [0, N) = D(seg), [N, 2N) = D(fake))
            self.tapes = {"G": tG, "D_real": D.slice_tape(tDq, 0, N) if stack else tDr, "D_fake": tDf}
        return self.gen_loss, self.disc_loss

    def _apply_gradients(self, *updates):
        """(optimizer, its network's all-reduce handle or None) in update order: each Adam launch waits for that network's
        gradient exchange only, so the exchanges still in flight run under the updates in front of them.  A guarded update
        (clip_grad_norm / skip_nonfinite) measures the buffer AFTER the exchange: every rank sees the same summed bits and
        1 / world enters the norm as grad_scale, so all ranks take the same decision without another collective.  A spectrally
        normalised discriminator's buffer holds gradients with respect to W / sigma until here: the transform to gradients with
        respect to W is linear, so it runs once on the exchanged buffer (every rank holds the same W, u, v and sigma), after any
        deferred weight gradient and directly before the update -- the guard measures the transformed gradient."""
        scale = 1.0 / self._world
        for opt, h in updates:
            if h is not None:
                h.wait()
            if _spectral_state(opt.net) is not None:
                opt.net.flush_wgrads()
                opt.net.spectral_grad()
            opt.apply_gradients(grad_scale=scale)

    def set_lr_schedule(self, steps_per_epoch, epoch_step, epochs):
        """The decay's parameters (``lr_decay`` models only): the base rate until epoch ``epoch_step``, then linearly down to 0
        at epoch ``epochs`` (model.py:223), where an optimizer's epoch is its ``iterations // steps_per_epoch`` -- so a run
        resumed from a checkpoint goes on decaying where it stopped.  Only writes the device descriptor the updates read:
        recorded steps follow it without being recorded again."""
        if self._lr_sched is None:
            raise RuntimeError("set_lr_schedule: this model was built without lr_decay")
        sched = (max(int(steps_per_epoch), 1), int(epoch_step), int(epochs))
        self._lr_sched.copy_(torch.tensor(sched, dtype=torch.int64))
        self._lr_sched_host = sched
        return self

    def networks(self):
        return (self.generator, self.discriminator) + ((self.generator_BA, self.discriminator_B) if self.cycle else ())

    def _net_names(self):
        return ("G", "D", "G_BA", "D_B") if self.cycle else ("G", "D")

    @property
    def guarded(self):
        return self.clip_grad_norm > 0 or self.skip_nonfinite

    def _ema_nets(self):
        return (self.generator, self.generator_BA) if self.cycle else (self.generator,)

    @contextlib.contextmanager
    def ema_weights(self):
        """Run the generators on the moving average of their weights (``ema_decay`` models only): on entry each generator's
        ``P.flat`` and ``P.ema`` change contents (K.swap_, one pass, bit for bit) and ``P.version`` is bumped so the packed
        operands are rebuilt; on exit they change back.  The trained weights return with every bit, so a step after the
        context -- eager or replayed from a recording made before it -- is the step it would have been.  Data parallel:
        nothing to exchange; every rank holds the same average, because every rank applies the same updates."""
        if self.ema_decay is None:
            raise RuntimeError("ema_weights: this model was built without ema_decay")
        def swap():
            for net in self._ema_nets():
                K.swap_(net.P.flat, net.P.ema)
                net.P.version += 1
        swap()
        try:
            yield self
        finally:
            swap()

    def _test_weights(self):
        """The weights the test passes run on: the average where the model keeps one, else the parameters as they are."""
        return self.ema_weights() if self.ema_decay is not None else contextlib.nullcontext()

    def grad_stats(self):
        """The guarded updates' records, {"G": {"norm", "clip", "skipped", "applied"}, "D": ...}: the last step's global
        gradient norm and clip factor and the running totals of skipped and applied updates per network.  ONE synchronising
        read -- for epoch ends and tests, not for the step.  Networks that never took a guarded step report zeros (clip 1)."""
        nets = self.networks()
        recs = [n.P._guard for n in nets]
        host = torch.stack([r for r in recs if r is not None]).cpu().tolist() if any(r is not None for r in recs) else []
        out, k = {}, 0
        for name, r in zip(self._net_names(), recs):
            row = [0.0, 1.0, 0.0, 0.0]
            if r is not None:
                row, k = host[k], k + 1
            out[name] = {"norm": row[0], "clip": row[1], "skipped": int(row[2]), "applied": int(row[3])}
        return out

    def _train_step_cycle(self):
        """2G+2D step assembled from the reference's defined-not-wired criteria (deviation D5):
        generator_loss / discriminator_loss (model.py:114-133) with criterionGAN = mae_criterion (--use_lsgan) or
        sce_criterion, abs_criterion cycle terms x --L1_lambda, gradloss_criterion x --Lg_lambda weighted by the
        segmentation-edge indicator (model.py:108-119).  Fakes in domain B are judged on A's mask and vice versa."""
        if self.paired and not self.use_pool and not self.mixed:
            return self._train_step_cycle_paired()
        Gab, Gba, Da, Db = self.generator, self.generator_BA, self.discriminator, self.discriminator_B
        rA, rB = self._prep(self.real_A), self._prep(self.real_B)
        sA, sB = self._prep(self.seg_A), self._prep(self.seg_B)
        mA, mB = self._convert_input("mask_A", self.mask_A), self._convert_input("mask_B", self.mask_B)
        for net in (Gab, Gba, Da, Db):
            net.P.zero_grad()
        Da.spectral_step(); Db.spectral_step()      # (d_norm="spectral": this step's sigma, before their first use)
        C = self.output_c_dim

        nA = rA.shape[0]
        fake_B, t1 = Gab.forward(rA, **self._drop(0, nA))
        cyc_A, t4 = Gba.forward(fake_B, **self._drop(1, nA))
        fake_A, t3 = Gba.forward(rB, **self._drop(0, nA))
        cyc_B, t2 = Gab.forward(fake_A, **self._drop(1, nA))
        aug = bool(self.diffaug)
        aBf, aAf, aAr, aBr = fake_B, fake_A, rA, rB                      # what the discriminators judge
        if aug:         # (never with the pool: refused by the constructor)
            n = rA.shape[0]
            par = self._diffaug_table(n, rA.shape[1], rA.shape[2], ((Db, 1, 0), (Db, 1, 1), (Da, 0, 1), (Da, 0, 0)))
            pBr, pBf, pAf, pAr = par[:n], par[n:2 * n], par[2 * n:3 * n], par[3 * n:]
            aBf, aAf = K.diffaug(fake_B, pBf, C), K.diffaug(fake_A, pAf, C)
            aAr, aBr = K.diffaug(rA, pAr, C), K.diffaug(rB, pBr, C)
        DB_fake, tDBf = Db.forward(aBf, mA)
        DA_fake, tDAf = Da.forward(aAf, mB)
        wA, wB = K.seg_edge_weight(sA, C), K.seg_edge_weight(sB, C)

        crit = K.mse_const if self.use_lsgan else K.bce_logits
        gl, dl = self._loss[0:1], self._loss[1:2]
        e = torch.empty_like
        gA_g, gB_g = e(DA_fake), e(DB_fake)                  # d g_loss / d logits
        crit(DA_fake, 1.0, gl, gA_g)
        crit(DB_fake, 1.0, gl, gB_g, accumulate_loss=True)
        d_cycA, d_cycB = e(cyc_A), e(cyc_B)
        K.l1_loss(rA, cyc_A, C, gl, d_cycA, weight=self.L1_lambda, accumulate=True)
        self._ssim_term(rA, cyc_A, C, gl, d_cycA)
        K.l1_loss(rB, cyc_B, C, gl, d_cycB, weight=self.L1_lambda, accumulate=True)
        self._ssim_term(rB, cyc_B, C, gl, d_cycB)
        d_fA, d_fB = e(fake_A), e(fake_B)                    # gradient-sensitive terms write, the rest accumulate
        K.gradloss(fake_A, rB, wB, C, gl, d_fA, lam=self.Lg_lambda, accumulate_loss=True)
        K.gradloss(fake_B, rA, wA, C, gl, d_fB, lam=self.Lg_lambda, accumulate_loss=True)
        # the discriminators judge a HISTORY of fakes when the image pool is on (utils.py:27-53); the pool returns the
        # current fakes until it is full, and then (p = 1/2) older ones, which need their own D forward
        pooled_A = pooled_B = False
        pfA = pfB = smA = smB = None
        if self.use_pool:
            pfA, pfB, smB, smA = self.pool([fake_A, fake_B, mB, mA])       # fake_A is judged on mask_B, fake_B on mask_A
            pooled_A, pooled_B = pfA is not fake_A, pfB is not fake_B      # (static pool: always fresh tensors -> always the stacked pass)
            assert not self.pool_static or self.batch_d_real_fake
        # D's two loss terms.  When the pool hands back older fakes they need their own D forward anyway: it is run
        # together with the real batch as ONE pass over 2N images (instance norm is per image, so this is exact) --
        # half the launches, and D's small tail layers (5x13 ... 1x5 maps) fill more of the chip.
        def d_loss_pass(Dn, real, m_real, DR, tR, pooled, fakes, m_fakes, DF, tF, first):
            if pooled and self.batch_d_real_fake:
                out, tape = Dn.forward(torch.cat([real, fakes]), torch.cat([m_real, m_fakes]))
                n = real.shape[0]
                grad = e(out)
                crit(out[:n], 1.0, dl, grad[:n], weight=0.5, accumulate_loss=not first)
                crit(out[n:], 0.0, dl, grad[n:], weight=0.5, accumulate_loss=True)
                Dn.backward(tape, grad)
                return
            if pooled:
                DF, tF = Dn.forward(fakes, m_fakes)
            g_r, g_f = e(DR), e(DF)
            crit(DR, 1.0, dl, g_r, weight=0.5, accumulate_loss=not first)
            crit(DF, 0.0, dl, g_f, weight=0.5, accumulate_loss=True)
            Dn.backward(tR, g_r); Dn.backward(tF, g_f)

        # discriminator gradients (fakes are constants here)
        if pooled_A and self.batch_d_real_fake:
            d_loss_pass(Da, rA, mA, None, None, True, pfA, smB, None, None, True)
        else:
            DA_real, tDAr = Da.forward(aAr, mA)
            d_loss_pass(Da, rA, mA, DA_real, tDAr, pooled_A, pfA if pooled_A else None, smB if pooled_A else None, DA_fake, tDAf, True)
        hDa = self._allreduce(Da)
        if pooled_B and self.batch_d_real_fake:
            d_loss_pass(Db, rB, mB, None, None, True, pfB, smA, None, None, False)
        else:
            DB_real, tDBr = Db.forward(aBr, mB)
            d_loss_pass(Db, rB, mB, DB_real, tDBr, pooled_B, pfB if pooled_B else None, smA if pooled_B else None, DB_fake, tDBf, False)
        hDb = self._allreduce(Db)
        # generator gradients: cycle terms first (they reach the other generator through the fakes).  Each generator is
        # applied twice, so the weight gradients of its 3x3 layers are paired: deferred here, launched with the second pass
        Gab.pair_wgrads = Gba.pair_wgrads = self.pair_wgrads
        # (the gradient joins ride on the first layer's data-gradient store -- ``addend`` -- instead of separate passes)
        d_fB = Gba.backward(t4, d_cycA, want_dx=True, addend=d_fB)
        d_fA = Gab.backward(t2, d_cycB, want_dx=True, addend=d_fA)
        if aug:         # through the transform's adjoint, which takes over the join
            d_fB = K.diffaug_bwd(Db.backward(tDBf, gB_g, want_dx=True, param_grads=False), pBf, C, addend=d_fB)
            d_fA = K.diffaug_bwd(Da.backward(tDAf, gA_g, want_dx=True, param_grads=False), pAf, C, addend=d_fA)
        else:
            d_fB = Db.backward(tDBf, gB_g, want_dx=True, param_grads=False, addend=d_fB)
            d_fA = Da.backward(tDAf, gA_g, want_dx=True, param_grads=False, addend=d_fA)
        hook, (hGba,) = self._bucketed_allreduce((Gba,))
        Gba.backward(t3, d_fA, on_unit_done=hook)               # second application: the paired weight gradients run here
        Gba.flush_wgrads(); Gba.pair_wgrads = False             # (nothing is left to flush unless a partner never came)
        hook, (hGab,) = self._bucketed_allreduce((Gab,))
        Gab.backward(t1, d_fB, on_unit_done=hook)
        Gab.flush_wgrads(); Gab.pair_wgrads = False

        self._apply_gradients((self.d_optim, hDa), (self.d_optim_B, hDb), (self.g_optim_BA, hGba), (self.g_optim, hGab))
        self.fake_A, self.fake_B = _LazyUnpad(fake_A, self.input_c_dim), _LazyUnpad(fake_B, C)
        self.cyc_A, self.cyc_B = _LazyUnpad(cyc_A, self.input_c_dim), _LazyUnpad(cyc_B, C)
        return self.gen_loss, self.disc_loss

    def _train_step_cycle_paired(self):
        """The cycle step with the symmetric halves of the objective in lockstep: every activation tensor stacks the two
        translation directions on the batch dimension -- [real_A; real_B] -> [fake_B; fake_A] -> [cyc_A; cyc_B] through
        (G_A->B, G_B->A) then (G_B->A, G_A->B); the fakes through (D_B, D_A), the reals through (D_A, D_B).  Convolutions still
        run per network; instance norms, activations and gradient joins run once per pair over twice the bytes.  Same kernels
        per image as _train_step_cycle: with ``d_quad=False`` losses, images and data gradients are bit-identical to it; weight
        gradients of layers whose two networks share a launch (sgg_conv2d_bwd_weight_pair2 and the all-taps / LDS-DMA shapes of
        sgg_conv2d_bwd_weight_group2: half as many split slabs per network) are equal up to f32 summation order (held to 1e-5
        of the tensor norm by the tests).  With ``d_quad`` (the default) the discriminators see reals and fakes as one 4N pass,
        whose small layers take other split-K plans than two 2N passes: the same mathematics in another f32 summation order
        (both forms are held to the float64 restatement at 2e-4 on every gradient tensor, tests/test_gpu_step.py)."""
        Gab, Gba, Da, Db = self.generator, self.generator_BA, self.discriminator, self.discriminator_B
        if getattr(self, "_pairs", None) is None:
            GP = GeneratorPair if self.arch == "resnet" else GeneratorUNetPair
            self._pairs = (GP(Gab, Gba), GP(Gba, Gab), DiscriminatorPair(Db, Da), DiscriminatorPair(Da, Db))
        Gp1, Gp2, Dpf, Dpr = self._pairs
        # Discriminators.  d_quad: reals AND fakes go through (D_B, D_A) as ONE stacked pass [real_B; fake_B | fake_A; real_A] --
        # half the launches of the two passes it replaces (the discriminators' tails are launch-latency bound) and the weight
        # gradients of both applications in one launch; the generators' loss backpropagates through the middle (fake) slice.
        # The stacked batches are persistent buffers: the inputs are converted straight into their slices and the generators'
        # last layer writes [fake_B; fake_A] into the middle of the discriminators' input -- nothing is concatenated.
        quad = self.d_quad
        shp = tuple(self.real_A.shape)
        n = shp[0]
        lo, hi = slice(0, n), slice(n, 2 * n)
        act_shape = tuple(shp[1:3]) + (K.cpad(self.input_c_dim),)
        x1 = self._stacked("x1", (2 * n,) + act_shape, self.dtype)
        rA, rB = self._prep(self.real_A, out=x1[lo]), self._prep(self.real_B, out=x1[hi])
        sA, sB = self._prep(self.seg_A), self._prep(self.seg_B)
        mA, mB = self._convert_input("mask_A", self.mask_A), self._convert_input("mask_B", self.mask_B)
        dq = None
        if quad:
            dq = self._stacked("dq", (4 * n,) + act_shape, self.dtype)
            self._prep(self.real_B, out=dq[:n]); self._prep(self.real_A, out=dq[3 * n:])
            mq = torch.cat([mB, mA, mB, mA], out=self._stacked("mq", (4 * n,) + tuple(mA.shape[1:]), mA.dtype))
            m_ab = mq[n:3 * n]                                # [mask_A; mask_B]
        else:
            m_ab = torch.cat([mA, mB])
        for net in (Gab, Gba, Da, Db):
            net.P.zero_grad()
        Da.spectral_step(); Db.spectral_step()      # (d_norm="spectral": this step's sigma, before their first use)
        C = self.output_c_dim
        f1, t1 = Gp1.forward(x1, out=dq[n:3 * n] if quad else None, **self._drop(0, n))   # [fake_B; fake_A]
        c2, t2 = Gp2.forward(f1, **self._drop(1, n))          # [cyc_A; cyc_B]
        aug = bool(self.diffaug)
        if aug:         # the discriminators judge augmented copies, rows in the stacked pass's order [real_B; fake_B | fake_A; real_A]
            par = self._diffaug_table(n, shp[1], shp[2], ((Db, 1, 0), (Db, 1, 1), (Da, 0, 1), (Da, 0, 0)))
            dq_aug = self._stacked("dq_aug", ((4 if quad else 2) * n,) + act_shape, self.dtype)
        if quad:
            Dq, tDq = Dpf.forward(K.diffaug(dq, par, C, out=dq_aug) if aug else dq, mq)
            Df, tDf = Dq[n:3 * n], Dpf.slice_tape(tDq, n, 3 * n)
        else:
            Df, tDf = Dpf.forward(K.diffaug(f1, par[n:3 * n], C, out=dq_aug) if aug else f1, m_ab)   # [D_B(fake_B | mask_A); D_A(fake_A | mask_B)]
        wA, wB = K.seg_edge_weight(sA, C), K.seg_edge_weight(sB, C)

        crit = K.mse_const if self.use_lsgan else K.bce_logits
        gl, dl = self._loss[0:1], self._loss[1:2]
        e = torch.empty_like
        g_g = e(Df)                                           # d g_loss / d logits, stacked like Df
        crit(Df[hi], 1.0, gl, g_g[hi])                        # D_A(fake_A)   (the loss terms in _train_step_cycle's order)
        crit(Df[lo], 1.0, gl, g_g[lo], accumulate_loss=True)  # D_B(fake_B)
        d_cyc = e(c2)
        K.l1_loss(rA, c2[lo], C, gl, d_cyc[lo], weight=self.L1_lambda, accumulate=True)
        self._ssim_term(rA, c2[lo], C, gl, d_cyc[lo])
        K.l1_loss(rB, c2[hi], C, gl, d_cyc[hi], weight=self.L1_lambda, accumulate=True)
        self._ssim_term(rB, c2[hi], C, gl, d_cyc[hi])
        d_f = e(f1)                                           # gradient-sensitive terms write, the rest accumulate
        K.gradloss(f1[hi], rB, wB, C, gl, d_f[hi], lam=self.Lg_lambda, accumulate_loss=True)
        K.gradloss(f1[lo], rA, wA, C, gl, d_f[lo], lam=self.Lg_lambda, accumulate_loss=True)

        # discriminator gradients (fakes are constants here): reals through (D_A, D_B), fakes through (D_B, D_A)
        tDr = None
        if quad:
            g_q = e(Dq)                                       # [real_B; fake_B | fake_A; real_A], the loss terms in the same order as below
            crit(Dq[3 * n:], 1.0, dl, g_q[3 * n:], weight=0.5, accumulate_loss=False)
            crit(Dq[2 * n:3 * n], 0.0, dl, g_q[2 * n:3 * n], weight=0.5, accumulate_loss=True)
            crit(Dq[:n], 1.0, dl, g_q[:n], weight=0.5, accumulate_loss=True)
            crit(Dq[n:2 * n], 0.0, dl, g_q[n:2 * n], weight=0.5, accumulate_loss=True)
            Dpf.backward(tDq, g_q)
        else:
            x1d = x1
            if aug:
                x1d = self._stacked("x1_aug", (2 * n,) + act_shape, self.dtype)
                K.diffaug(x1[lo], par[3 * n:], C, out=x1d[lo]); K.diffaug(x1[hi], par[:n], C, out=x1d[hi])
            Dr, tDr = Dpr.forward(x1d, m_ab)                  # [D_A(real_A | mask_A); D_B(real_B | mask_B)]
            g_r, g_fk = e(Dr), e(Df)
            crit(Dr[lo], 1.0, dl, g_r[lo], weight=0.5, accumulate_loss=False)
            crit(Df[hi], 0.0, dl, g_fk[hi], weight=0.5, accumulate_loss=True)
            crit(Dr[hi], 1.0, dl, g_r[hi], weight=0.5, accumulate_loss=True)
            crit(Df[lo], 0.0, dl, g_fk[lo], weight=0.5, accumulate_loss=True)
            Dpr.backward(tDr, g_r)
            Dpf.backward(tDf, g_fk)
        hDa, hDb = self._allreduce(Da), self._allreduce(Db)
        # generator gradients: cycle terms first (they reach the other generator through the fakes).  Each generator is applied
        # twice, so the weight gradients of its 3x3 layers are paired: deferred in the first pass, launched with the second
        Gab.pair_wgrads = Gba.pair_wgrads = self.pair_wgrads
        # (the gradient joins ride on the first layer's data-gradient store -- ``addend`` -- instead of separate passes)
        d_f = Gp2.backward(t2, d_cyc, want_dx=True, addend=d_f)
        if aug:         # through the transform's adjoint, which takes over the join
            d_f = K.diffaug_bwd(Dpf.backward(tDf, g_g, want_dx=True, param_grads=False), par[n:3 * n], C, addend=d_f)
        else:
            d_f = Dpf.backward(tDf, g_g, want_dx=True, param_grads=False, addend=d_f)
        # second application of both generators: every deferred weight gradient runs inside this pass, and each layer group's
        # all-reduce is launched as soon as the group is complete -- only the last group's exchange has no backward work left
        # to hide behind (the four Adam launches run under it)
        hook, (hGab, hGba) = self._bucketed_allreduce((Gab, Gba))
        Gp1.backward(t1, d_f, on_unit_done=hook)
        assert self._dp is None or not (Gab.pending_wgrads() or Gba.pending_wgrads())   # (their buckets are already travelling)
        Gba.flush_wgrads(); Gab.flush_wgrads()                  # (nothing is left to flush unless a partner never came)
        Gab.pair_wgrads = Gba.pair_wgrads = False

        self._apply_gradients((self.d_optim, hDa), (self.d_optim_B, hDb), (self.g_optim_BA, hGba), (self.g_optim, hGab))
        self.fake_A, self.fake_B = _LazyUnpad(f1[hi], self.input_c_dim), _LazyUnpad(f1[lo], C)
        self.cyc_A, self.cyc_B = _LazyUnpad(c2[lo], self.input_c_dim), _LazyUnpad(c2[hi], C)
        if self.keep_tapes:
            # stacked [first network's images; second network's images] -- see the docstring.  d_quad: "D_quad" is the ONE
            # discriminator pass [D_B(real_B); D_B(fake_B) | D_A(fake_A); D_A(real_A)] and "D_fake" its middle slice (views);
            # otherwise "D_fake" = [D_B(fake_B); D_A(fake_A)] and "D_real" = [D_A(real_A); D_B(real_B)] are the two passes
            self.tapes = {"G_first": t1, "G_second": t2, "D_fake": tDf, "D_real": tDr, "D_quad": tDq if quad else None, "n": n}
        return self.gen_loss, self.disc_loss

    # ------------------------------------------------------------------ convenience
    def losses(self):
        """Host copies of (gen_loss, disc_loss) -- the two scalars model.py:260 prints."""
        v = self._loss.detach().cpu().tolist()
        return v[0], v[1]

    def state_dict(self):
        sd = {}
        names = ("G", "D", "G_BA", "D_B") if self.cycle else ("G", "D")
        for key, net in zip(names, self.networks()):
            P = net.P
            sd[key] = {"flat": P.flat.cpu(), "m": P.m.cpu(), "v": P.v.cpu(), "t": P.step_count}
            if P._guard is not None:            # the guarded update's counters [skipped_total, applied_total]
                sd[key]["guard"] = [int(c) for c in P._guard[2:4].cpu().tolist()]
            if P.ema is not None:               # the moving average of the generator's parameters (ema_decay)
                sd[key]["ema"] = P.ema.cpu()
            if _spectral_state(net) is not None:    # a spectrally normalised discriminator: its kind and its power-iteration vectors
                sd[key]["d_norm"], sd[key]["u"] = "spectral", _spectral_state(net).cpu()
        sd["G"]["arch"] = self.arch             # generator architecture tag (a checkpoint without one is a ResNet checkpoint)
        mine = getattr(self, "upsample", "deconv")
        if mine != "deconv":                    # how d1 / d2 double the resolution (a checkpoint without the tag: transposed convs)
            for key in names[0::2]:
                sd[key]["upsample"] = mine
        return sd

    def load_state_dict(self, sd):
        names = ("G", "D", "G_BA", "D_B") if self.cycle else ("G", "D")
        arch = sd["G"].get("arch", "resnet")
        if arch != self.arch:
            raise ValueError(f"checkpoint holds a {arch} generator, this model is built with a {self.arch} generator "
                             f"(--generator {self.arch}); load it into a model built with --generator {arch}")
        for key in names[0::2]:                 # (before anything is copied)
            kind, mine = sd[key].get("upsample", "deconv"), getattr(self, "upsample", "deconv")
            if kind != mine:
                raise ValueError(f"checkpoint holds a generator whose d1 / d2 are built with --upsample {kind}, this model is built "
                                 f"with --upsample {mine}; load it into a model built with --upsample {kind}")
        for key in names[1::2]:
            kind = sd[key].get("d_norm", "instance")
            mine = getattr(self, "d_norm", "instance")
            if kind != mine:
                raise ValueError(f"checkpoint holds {kind}-norm discriminators, this model is built with {mine}-norm "
                                 f"discriminators (--d_norm {mine}); load it into a model built with --d_norm {kind}")
        for key, net in zip(names, self.networks()):
            P = net.P
            P.flat.copy_(sd[key]["flat"]); P.m.copy_(sd[key]["m"]); P.v.copy_(sd[key]["v"])
            P.step_count = int(sd[key]["t"]); P.version += 1
            if _spectral_state(net) is not None:
                u = sd[key].get("u")
                if u is None and not self._sn_notice:
                    self._sn_notice = True
                    print(" [*] spectral-norm checkpoint without power-iteration vectors: they start from the seeded ones")
                net.set_spectral_state(u)
            counters = sd[key].get("guard")     # (absent from a checkpoint of a run without the options)
            if counters is not None:
                P.guard_buffers()[0][2:4].copy_(torch.tensor([float(c) for c in counters], dtype=torch.float64))
            elif P._guard is not None:
                P._guard[2:4].zero_()
            if P.ema is not None:               # (a model without ema_decay ignores the key)
                ema = sd[key].get("ema")
                if ema is None and not self._ema_notice:
                    self._ema_notice = True
                    print(" [*] checkpoint without a weight average: the average starts from the loaded weights")
                P.ema.copy_(sd[key]["flat"] if ema is None else ema)

    def _ckpt_paths(self, checkpoint_dir, ep=None):
        """model.py:454-456: <checkpoint_dir>/<dataset_dir>/{gen,disc}/cp-{epoch:04d}.ckpt"""
        base = os.path.join(checkpoint_dir, self.dataset_dir)
        f = (lambda sub: os.path.join(base, sub, "cp-%04d.ckpt" % ep)) if ep is not None else (lambda sub: os.path.join(base, sub))
        return f("gen"), f("disc")

    def save(self, checkpoint_dir, ep):
        """model.py:450-468 (weights per network under gen/ and disc/), plus what the reference omits: the Adam
        slots and step counts, so training resumes exactly (SURVEY.md 5 "Checkpoint / resume")."""
        gpath, dpath = self._ckpt_paths(checkpoint_dir, ep)
        sd = self.state_dict()
        for path, keys in ((gpath, ("G", "G_BA")), (dpath, ("D", "D_B"))):
            os.makedirs(os.path.dirname(path), exist_ok=True)
            torch.save({k: sd[k] for k in keys if k in sd}, path)
        return gpath, dpath

    def load(self, checkpoint_dir):
        """model.py:471-503: load the latest gen/disc checkpoints; False if either is missing."""
        import glob
        gdir, ddir = self._ckpt_paths(checkpoint_dir)
        lg, ld = sorted(glob.glob(gdir + "/cp-*.ckpt")), sorted(glob.glob(ddir + "/cp-*.ckpt"))
        if not (lg and ld):
            return False
        sd = {}
        sd.update(torch.load(lg[-1], map_location="cpu"))
        sd.update(torch.load(ld[-1], map_location="cpu"))
        self.load_state_dict(sd)
        return True

    def get_labels(self, test_label, pred_img, crf=False):
        """model.py:278-305: (lt, lp) for the label plots.  crf=False: both transposed to (N,C,W,H) (model.py:302-303).
        crf=True (crf_wrapper, model.py:282-296): lt = uint8(255 * test_label) as it is, lp = dense_crf(lt[0], pred_img
        transposed to (C,W,H)) with a leading axis of one; like the reference's call this needs H == W."""
        from . import metric as M
        as_np = lambda x: x.numpy() if hasattr(x, "numpy") else np.asarray(x)
        if crf:
            image = (as_np(test_label) * 255).astype(np.uint8)
            lp = as_np(pred_img).transpose(0, 3, 2, 1)[0]
            return image, np.expand_dims(M.dense_crf(image[0], lp), axis=0)
        return as_np(test_label).transpose(0, 3, 2, 1), as_np(pred_img).transpose(0, 3, 2, 1)

    def test_during_train(self, epoch, args, samples, sink=None, swd_reals=None):
        """model.py:307-448 (the live part): every test sample -- ``samples`` yields (name, sample_image (H,W,3) in [0,1], seg_image (H,W,3)
        in [0,1][, one-hot class mask (H,W,C)]); reading and resizing the files stays with the caller -- is translated, optionally saved under
        ``args.test_dir``, and scored (evaluate.py) by the reference's FCN scores and by the scorers that ``args.crf`` / ``class_scores`` /
        ``image_scores`` / ``swd`` name, which need their element of EVERY sample.  Returns (the stacked fakes as model.py:440-448, the scores)."""
        optional = {"crf": E.CrfLabels(args.segment_class),
                    "class_scores": E.ClassHists(args, self.device, int(getattr(args, "boundary_px", 3)), getattr(args, "crf", False)),
                    "image_scores": E.ImageQuality(self.generator_BA if self.cycle else None), "swd": E.Swd(self, args, swd_reals)}
        scorers = [E.SegLabels(args.segment_class)] + [sc for option, sc in optional.items() if getattr(args, option, False)]
        def each(s):
            if getattr(args, "test_dir", None):
                os.makedirs(args.test_dir, exist_ok=True)
                save_images(s.fake, [1, 1], os.path.join(args.test_dir, os.path.basename(s.name)))     # :362-365
            return s.fake_img
        outputs, results = E.run(self, samples, scorers, each, strict=True)
        score = {k: v for res in results for k, v in res.items()}
        if sink is not None:                                                                         # :389-393
            decay = float(self.generator.P._ema_state[0].item()) if self.ema_decay is not None else None
            for tag, value in E.scalars(score, decay):
                sink.scalar(tag, value, epoch)
        return (np.concatenate(outputs, axis=0) if outputs else None), score

    def test(self, args, samples, log=print):
        """model.py:535-567 (--phase test): load the latest checkpoint, translate every test sample -- (name, sample_image (H,W,3) in [0,1][, label
        image[, one-hot class mask]]) --, save the input and the translation under ``args.test_dir``; the scorers (evaluate.py) of ``class_scores``
        ("Class" alone), ``image_scores`` and ``swd`` (``args.swd_reals`` where set) score the samples that carry what they need.  Returns the fakes."""
        optional = {"class_scores": E.ClassHists(args, self.device), "image_scores": E.ImageQuality(),
                    "swd": E.Swd(self, args, getattr(args, "swd_reals", None))}
        scorers = [sc for option, sc in optional.items() if getattr(args, option, False)]
        log(" [*] Running Test ...")
        log(" [*] Load SUCCESS" if self.load(args.checkpoint_dir) else " [!] Load failed...")
        os.makedirs(args.test_dir, exist_ok=True)
        def each(s):
            log("Processing image: " + s.name)
            save_images(s.image[None], [1, 1], os.path.join(args.test_dir, "real_" + os.path.basename(s.name)))
            save_images(s.fake, [1, 1], os.path.join(args.test_dir, os.path.basename(s.name)))
            return s.fake
        out, results = E.run(self, samples, scorers, each, strict=False)
        for res in results:
            log(" ".join("%s: %f" % tv for tv in E.scalars(res)))
        return out

    def train(self, args, batches, log=print, test_samples=None, sink=None):
        """The reference's epoch loop (model.py:202-275) around ``train_step`` for a caller-supplied batch source:
        ``batches(epoch)`` yields dicts with real_A / seg_A / mask_A (+ real_B / seg_B / mask_B in cycle mode) --
        data.DirectoryBatches loads them from a dataset directory (utils.py:167-233), any other source is the caller's; ``test_samples`` / ``sink`` add the epoch-end
        test pass and the scalar summaries of model.py:263-268.  Prints the reference's line
        (model.py:260), keeps its running-mean loss metrics (model.py:23-24,193-194,270-271), honours
        --continue_train (model.py:210-215) and saves in ``finally`` like model.py:272-275."""
        import time
        start = time.time()
        if getattr(args, "continue_train", False):
            log(" [*] Loading pretrained weights ...")
            log(" [*] Load SUCCESS" if self.load(args.checkpoint_dir) else " [!] Load failed...")
        else:
            log(" [*] New training STARTED")
        history, epoch = [], 0
        try:
            for epoch in range(args.epoch):
                self.gen_loss_metric = self.disc_loss_metric = self.fm_loss_metric = 0.0
                self._metric_n = 0
                data = batches(epoch)
                if not hasattr(data, "__len__"):       # a sized source (data.DirectoryBatches) refills its buffers per step: keep it lazy
                    data = list(data)
                if self.lr_decay:
                    self.set_lr_schedule(len(data), args.epoch_step, args.epoch)
                for idx, b in enumerate(data):
                    for k, v in b.items():
                        setattr(self, k, v)
                    self.train_step(args)
                    gl, dl = self.losses()
                    self._metric_n += 1
                    self.gen_loss_metric += (gl - self.gen_loss_metric) / self._metric_n
                    self.disc_loss_metric += (dl - self.disc_loss_metric) / self._metric_n
                    line = "Epoch: [%2d] [%4d/%4d] time: %4.4f Gen_Loss: %f Disc_Loss: %f " % (epoch, idx, len(data), time.time() - start, gl, dl)
                    if self.fm_lambda:                 # the term itself (unweighted), read beside the two losses
                        fm = float(self.fm_loss.item())
                        self.fm_loss_metric += (fm - self.fm_loss_metric) / self._metric_n
                        line += "fm_loss: %f " % fm
                    log(line)
                # epoch end (model.py:263-268): the test pass + image summary, then the two running-mean loss scalars
                if test_samples is not None:
                    extra = {"swd_reals": args.swd_reals} if getattr(args, "swd", False) and getattr(args, "swd_reals", None) is not None else {}
                    fake, _ = self.test_during_train(epoch, args, test_samples(epoch) if callable(test_samples) else test_samples, sink,
                                                     **extra)
                    if sink is not None and fake is not None:
                        sink.image("Segmentation Epoch {}".format(epoch), fake, epoch)
                if sink is not None:
                    sink.scalar("Generator Loss", self.gen_loss_metric, epoch)
                    sink.scalar("Discriminator Loss", self.disc_loss_metric, epoch)
                    if self.fm_lambda:
                        sink.scalar("Feature Matching Loss", self.fm_loss_metric, epoch)
                    if self.lr_decay:              # the rate the generator's last update of this epoch applied
                        last = max(self.g_optim.iterations.item() - 1, 0)
                        sink.scalar("Learning Rate", float(K.scheduled_lr(self.g_optim.learning_rate, last, *self._lr_sched_host)), epoch)
                    if self.guarded:               # the last step's gradient norm and the skipped updates so far, per network
                        for name, st in self.grad_stats().items():
                            sink.scalar(name + " Grad Norm", st["norm"], epoch)
                            sink.scalar(name + " Skipped Updates", st["skipped"], epoch)
                history.append({"epoch": epoch, "Generator Loss": self.gen_loss_metric, "Discriminator Loss": self.disc_loss_metric})
        finally:
            if getattr(args, "checkpoint_dir", None):
                self.save(args.checkpoint_dir, epoch)
        return history


class _PendingReduce:
    """Handle of one network's gradient all-reduces (one per bucket): ``wait()`` orders the compute stream behind all of
    them (a host action, see _host)."""

    def __init__(self, model):
        self._model, self.works = model, []

    def wait(self):
        def wait_all():
            for w in self.works:
                w.wait()
            self.works.clear()
        self._model._host(wait_all)


class _LazyUnpad:
    """``self.fake_A``: the generator output kept in its internal layout; converts to the reference's
    (N,H,W,3) float32 on demand so the step itself does no extra pass."""

    def __init__(self, internal, c):
        self._t, self._c = internal, c

    def tensor(self):
        return K.unpad_channels(self._t, self._c)

    def numpy(self):
        return self.tensor().cpu().numpy()

    @property
    def shape(self):
        return tuple(self._t.shape[:-1]) + (self._c,)

    def __array__(self, dtype=None):
        a = self.numpy()
        return a if dtype is None else a.astype(dtype)
