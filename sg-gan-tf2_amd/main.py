"""Flag surface of the reference's ``main.py`` (main.py:14-43: same names, types and defaults -- SURVEY.md 8(f)3)
driving ``sggan`` on a dataset directory (data.py) or, where ``--dataset_dir`` names none, on synthetic batches.  The reference's quirks are kept as data, not behaviour: --lr, --L1_lambda
and friends are parsed but the live (reference-mode) step hard-codes lr=1e-3 and LAMBDA=100 (model.py:151,205);
they take effect in --cycle mode, which uses the criteria those flags were written for."""
from __future__ import annotations

import argparse
import os


def build_parser():
    p = argparse.ArgumentParser(description="")
    a = p.add_argument
    a("--dataset_dir", dest="dataset_dir", default="city")
    a("--epoch", dest="epoch", type=int, default=100)
    a("--epoch_step", dest="epoch_step", type=int, default=100)
    a("--batch_size", dest="batch_size", type=int, default=1)
    a("--train_size", dest="train_size", type=int, default=int(1e8))
    a("--img_height", dest="image_height", type=int, default=64)
    a("--img_width", dest="image_width", type=int, default=64)
    a("--ratio_gan2seg", dest="ratio_gan2seg", type=int, default=10)
    a("--use_augmentation", dest="use_augmentation", type=bool, default=True)
    a("--ngf", dest="ngf", type=int, default=64)
    a("--ndf", dest="ndf", type=int, default=64)
    a("--input_nc", dest="input_nc", type=int, default=3)
    a("--output_nc", dest="output_nc", type=int, default=3)
    a("--lr", dest="lr", type=float, default=0.0002)
    a("--beta1", dest="beta1", type=float, default=0.5)
    a("--which_direction", dest="which_direction", default="AtoB")
    a("--phase", dest="phase", default="train")
    a("--save_freq", dest="save_freq", type=int, default=1000)
    a("--print_freq", dest="print_freq", type=int, default=5)
    a("--continue_train", dest="continue_train", type=bool, default=False)
    a("--checkpoint_dir", dest="checkpoint_dir", default="./checkpoint")
    a("--sample_dir", dest="sample_dir", default="./sample")
    a("--test_dir", dest="test_dir", default="./test")
    a("--L1_lambda", dest="L1_lambda", type=float, default=10.0)
    a("--Lg_lambda", dest="Lg_lambda", type=float, default=5.0)
    a("--use_resnet", dest="use_resnet", type=bool, default=False)
    a("--use_lsgan", dest="use_lsgan", type=bool, default=True)
    a("--use_pix2pix", dest="use_pix2pix", type=bool, default=False)
    a("--max_size", dest="max_size", type=int, default=50)
    a("--segment_class", dest="segment_class", type=int, default=34)
    # build-specific knobs (not in the reference)
    a("--generator", dest="generator", choices=("resnet", "unet"), default="resnet",
      help="generator network: resnet (generator_resnet, this build's default) or unet (generator_unet: the reference's "
           "default, i.e. its flag-less --use_resnet False); either one trains in reference mode and with --cycle")
    a("--cycle", dest="cycle", action="store_true",
      help="2G+2D cycle-mode step (north_star unit): both generators are of the --generator kind and run in lockstep")
    a("--paired", dest="paired", type=int, choices=(0, 1), default=None,
      help="--cycle: 1 runs the two generators and the two discriminators in lockstep on stacked batches, 0 one network at a time; "
           "default: 1 for the ResNet, 0 for the U-Net (where lockstep only pays at small sizes, e.g. 128x128)")
    a("--dtype", dest="dtype", default="bf16")
    a("--steps_per_epoch", dest="steps_per_epoch", type=int, default=4)
    a("--use_pool", dest="use_pool", action="store_true",
      help="train the discriminators on utils.ImagePool's history of fakes (--max_size entries; upstream SG-GAN behaviour, cycle mode)")
    a("--graph", dest="graph", action="store_true", help="replay the step from captured HIP graphs")
    a("--checkpoint_blocks", dest="checkpoint_blocks", action="store_true",
      help="activation checkpointing: re-run each residual block in backward instead of keeping its activations")
    a("--dataset_dir_B", dest="dataset_dir_B", default=None,
      help="cycle mode: dataset root of domain B (its trainB* folders, else its trainA*); default: trainB* of --dataset_dir")
    a("--augment", dest="augment", action="store_true",
      help="train on every sample and its augmented copy (flip / crop / affine, 2 x batch_size images per step): the reference's "
           "default --use_augmentation branch; that flag is type=bool and cannot be switched off, so it stays inert")
    a("--crf", dest="crf", action="store_true",
      help="epoch-end test pass: also score dense_crf(test image, class mask) against the class mask (metric.scores_mask_sample_crf) "
           "and log the four scores as 'CRF ...' scalars; needs testA_seg_class beside testA")
    a("--lr_decay", dest="lr_decay", action="store_true",
      help="linear learning-rate decay, the rule --epoch_step was written for (model.py:223): "
           "lr if epoch < epoch_step else lr*(epoch_total-epoch)/(epoch_total-epoch_step), with epoch_total = --epoch and lr = --lr "
           "in --cycle mode (the reference-mode step's hard-coded 1e-3 otherwise); evaluated on the device from each optimizer's step "
           "counter (epoch = iterations // steps per epoch), so it survives graph replay and goes on after --continue_train")
    # (the two guard flags are absent from the namespace unless given -- sggan reads them with its own defaults, 0 and off --
    # so a run without them is configured by exactly the namespace it had before they existed)
    a("--clip_grad_norm", dest="clip_grad_norm", type=float, default=argparse.SUPPRESS,
      help="clip every network's gradient to this global L2 norm before its Adam update (default 0 = off); the norm is measured "
           "and the factor applied on the device by the update's own launches, so it costs no host sync and works under --graph; "
           "a gradient that holds a NaN or Inf is skipped, as with --skip_nonfinite")
    a("--skip_nonfinite", dest="skip_nonfinite", action="store_true", default=argparse.SUPPRESS,
      help="skip a network's update when its gradient holds a NaN or Inf: parameters, Adam slots and step counter keep their "
           "bits and the skip is counted ('<network> Skipped Updates' scalar at epoch end)")
    a("--ema_decay", dest="ema_decay", type=float, default=argparse.SUPPRESS,
      help="keep an exponential moving average of the generator weights with this decay (in (0, 1), e.g. 0.999; default: off) and "
           "run the epoch-end test pass and --phase test on the average; the average is updated inside the Adam launch with "
           "the ramp min(decay, (1 + t) / (10 + t)) over applied updates, so it works under --graph, leaves the average alone when "
           "an update is skipped, and goes on after --continue_train")
    # (absent from the namespace unless given, like the guard flags)
    a("--diffaug", dest="diffaug", metavar="POLICY", default=argparse.SUPPRESS,
      help="differentiable augmentation of everything the discriminators see (Zhao et al. 2020): 'color', 'cutout' or "
           "'color,cutout' (default: off).  The same random transform family is applied to reals and fakes in front of D and the "
           "generator's adversarial gradient flows back through it; the parameters are drawn on the device from D's step counter "
           "and the global sample index, so it works under --graph, with data parallelism and after --continue_train.  "
           "Translation is not offered (D's class mask cannot follow a shift); not with --use_pool")
    a("--diffaug_brightness", dest="diffaug_brightness", type=float, default=argparse.SUPPRESS,
      help="--diffaug color: width of the brightness shift, b = (u - 0.5) * this (default 0.25: images live in [0,1])")
    a("--ssim_lambda", dest="ssim_lambda", type=float, default=argparse.SUPPRESS,
      help="add X * (1 - mean SSIM) to the generators' loss beside every L1 reconstruction term (default 0 = off): with --cycle "
           "on (real_A, cyc_A) and (real_B, cyc_B), otherwise on (label image, fake).  SSIM as --image_scores measures it (11x11 "
           "Gaussian window, sigma 1.5, the windows inside the image) but on the float images, with its exact gradient, in double "
           "on the device; works under --graph, with data parallelism, --use_pool and --diffaug; training images must be at "
           "least 11 pixels high and wide")
    a("--ssim_data_range", dest="ssim_data_range", type=float, default=argparse.SUPPRESS,
      help="--ssim_lambda: the span of the image values that fixes SSIM's constants C1 = (0.01 R)^2, C2 = (0.03 R)^2 "
           "(default 1: the step's images live in [0,1])")
    a("--fm_lambda", dest="fm_lambda", type=float, default=argparse.SUPPRESS,
      help="paired (reference-mode) step: add X * the feature-matching term of pix2pixHD (Wang et al. 2018) to the generator's loss "
           "(default 0 = off): the mean over the discriminator's seven intermediate activations of mean |D_k(fake) - D_k(label "
           "image)|, from one call on the activations the discriminator pass already holds; the discriminator's own gradient "
           "never sees it (DESIGN.md 30).  Works under --graph, with data parallelism, both generators, --d_norm spectral, "
           "--ssim_lambda, --dropout, --upsample, the guard flags, --ema_decay, --augment and --lr_decay.  Refused with --cycle "
           "(no pixel-aligned real) and with --diffaug (independent draws for reals and fakes)")
    a("--d_norm", dest="d_norm", choices=("instance", "spectral"), default=argparse.SUPPRESS,
      help="normalisation of the discriminators (default instance, the reference's network).  spectral (Miyato et al. 2018): no "
           "discriminator layer has an instance norm -- it would cancel any scale of the kernel in front of it -- and every "
           "discriminator conv runs on W / sigma(W), sigma kept by one power iteration per discriminator per step on the device; "
           "the per-layer vectors are saved with the checkpoint, so it works under --graph, with data parallelism (nothing to "
           "exchange), --use_pool, the guard flags and after --continue_train; with --diffaug the draws stay keyed by the "
           "discriminator's step counter, unchanged.  A checkpoint loads only into a model of the same --d_norm")
    a("--dropout", dest="dropout", nargs="?", type=float, const=0.5, metavar="RATE", default=argparse.SUPPRESS,
      help="--generator unet: train the generator(s) with the Dropout layers of generator_unet (d1..d3, between the transposed conv and the "
           "instance norm) in training mode, at RATE in [0, 1) (bare flag: 0.5, the reference's constant; default: off -- the "
           "reference's own calls run the generator in inference mode).  The masks are regenerated on the device from the "
           "generator's step counter, the layer and the global sample index, never stored, so it works under --graph, with data "
           "parallelism and after --continue_train; the test passes stay in inference mode.  Refused with --generator resnet: that "
           "network has no dropout layers")
    a("--upsample", dest="upsample", choices=("deconv", "nearest", "bilinear"), default=argparse.SUPPRESS,
      help="how generator_resnet's two doubling layers d1 / d2 reach the next resolution (DESIGN.md 29): 'deconv' (default) -- the "
           "reference's stride-2 transposed 3x3 convs; 'nearest' | 'bilinear' -- a fixed 2x resampling followed by a 3x3 stride-1 "
           "SAME conv, the resize-convolution of Odena et al. 2016 against checkerboard artifacts (4x the layer's multiply-adds).  "
           "Same parameter count; a checkpoint loads only into a model of the same --upsample.  Refused with --generator unet")
    a("--class_scores", dest="class_scores", action="store_true", default=argparse.SUPPRESS,
      help="test pass: decode every translation to class labels through the palette learned from the test set's own (colour label, "
           "class map) pairs and score it against the class map: 'Class Overall Accuracy' ... 'Class Mean IoU' scalars, "
           "'Boundary Class Mean IoU' (--boundary_px) and, with --crf, the 'Class CRF ...' scores of the CRF-refined map; "
           "needs testA_seg_class beside testA; --segment_class is the class count")
    a("--boundary_px", dest="boundary_px", type=int, default=argparse.SUPPRESS,
      help="--class_scores: half-width in pixels (0..8, default 3) of the band around ground-truth class boundaries that "
           "'Boundary Class Mean IoU' is scored on; 0 leaves the scalar out")
    a("--class_max_dist", dest="class_max_dist", type=int, default=argparse.SUPPRESS,
      help="--class_scores: a pixel whose 8-bit colour is farther than this (Euclidean, RGB) from every palette colour counts as "
           "class 0 (default -1: always the nearest colour)")
    a("--image_scores", dest="image_scores", action="store_true", default=argparse.SUPPRESS,
      help="test pass: compare every translation, as the 8-bit image it is saved as, with the 8-bit label image: 'Image MAE', "
           "'Image PSNR' and 'Image SSIM' scalars (SSIM: 11x11 Gaussian window, sigma 1.5, the mean over the windows inside the "
           "image; computed in double on the GPU); with --cycle also 'Cycle MAE / PSNR / SSIM' of the reconstruction "
           "G_BA(G_AB(x)) against the input; images must be at least 11 pixels high and wide")
    a("--swd", dest="swd", action="store_true", default=argparse.SUPPRESS,
      help="test pass: the sliced Wasserstein distance of Laplacian-pyramid patches (Karras et al. 2018) between the translations "
           "and a set of real images, both taken as 8-bit images: 'SWD <h>x<w>' per pyramid level and 'SWD Mean' scalars "
           "(x 1e3, lower is closer).  An unpaired score: with --cycle on a dataset directory the reals are the first images "
           "of testB (else trainB) of domain B, otherwise the label images of the test samples.  The level count is the largest "
           "L <= 5 for which the test size divides by 2^(L-1) with min(H, W) >> (L-1) >= 16")
    a("--swd_patches", dest="swd_patches", type=int, default=argparse.SUPPRESS,
      help="--swd: 7x7 patches drawn per image and pyramid level (default 128)")
    a("--log_dir", dest="log_dir", default="./logs", help="scalar summaries (the reference writes tfevents under logs/<timestamp>/train)")
    return p


def synthetic_batches(model, args):
    import torch
    from .segment_class import one_hot_mask

    def gen(epoch):
        g = torch.Generator().manual_seed(19 + epoch)
        H, W, N = args.image_height, args.image_width, args.batch_size
        mh, mw = model.discriminator.out_hw(H, W)
        if (mh, mw) == (1, 1):
            mh, mw = round(H / 34), round(W / 34)
        for _ in range(args.steps_per_epoch):
            def dom():
                idx = torch.randint(0, args.segment_class, (N, max(H // 32, 1), max(W // 32, 1)), generator=g)
                idx = idx.repeat_interleave(H // idx.shape[1], 1).repeat_interleave(W // idx.shape[2], 2).to(torch.uint8)
                pal = torch.rand((args.segment_class, 3), generator=torch.Generator().manual_seed(7))
                return torch.rand((N, H, W, 3), generator=g), pal[idx.long()], one_hot_mask(idx, mh, mw, args.segment_class)
            rA, sA, mA = dom()
            b = {"real_A": rA, "seg_A": sA, "mask_A": mA}
            if args.cycle:
                rB, sB, mB = dom()
                b.update({"real_B": rB, "seg_B": sB, "mask_B": mB})
            yield b
    return gen


def synthetic_test_samples(args, count=2):
    """(name, sample_image, seg_image) triples in the reference loader's ranges (utils.load_test_data: floats in [0,1])."""
    import torch

    def gen(epoch=0):
        g = torch.Generator().manual_seed(1000 + epoch)
        H, W = args.image_height, args.image_width
        for i in range(count):
            item = ("synthetic_%03d.png" % i, torch.rand((H, W, 3), generator=g).numpy(), torch.rand((H, W, 3), generator=g).numpy())
            if getattr(args, "crf", False) or getattr(args, "class_scores", False):      # drawn after the triple (once for both
                # flags), so the triple is what it is without them
                idx = torch.randint(0, args.segment_class, (H, W), generator=g)
                item += (torch.nn.functional.one_hot(idx, args.segment_class).float().numpy(),)
            yield item
    return gen


def parse_args(argv=None):
    """build_parser().parse_args with --generator applied: it decides use_resnet (the reference's type=bool --use_resnet
    cannot be set to False from the command line; its flag-less default is the U-Net, ``--generator unet`` here)."""
    args = build_parser().parse_args(argv)
    args.use_resnet = args.generator == "resnet"
    return args


def directory_sources(model, args, log=print):
    """(batches, test_samples) from the dataset directory ``--dataset_dir`` names (as given, else ./datasets/<dataset_dir>:
    model.py:220), or None where it has no ``trainA`` folder (the caller then keeps the synthetic sources)."""
    from . import data as D
    root = D.resolve_root(args.dataset_dir)
    if root is None:
        return None
    augment = bool(getattr(args, "augment", False))
    if args.use_augmentation and not augment:
        log(" [*] --use_augmentation is inert here: pass --augment to train on every sample plus its augmented copy "
            "(flip / crop / affine of utils.py:80-103, 2 x batch_size images per step; DESIGN.md 11)")
    dev = model.device
    cache_A = D.DatasetCache(root, "trainA", device=dev, max_files=args.train_size)
    cache_B = None
    if args.cycle:
        root_B = root
        if args.dataset_dir_B:
            root_B = D.resolve_root(args.dataset_dir_B, "trainB") or D.resolve_root(args.dataset_dir_B, "trainA")
        split_B = "trainB" if root_B and os.path.isdir(os.path.join(root_B, "trainB")) else "trainA"
        if root_B is None or (not args.dataset_dir_B and split_B == "trainA"):
            raise FileNotFoundError("--cycle needs a second domain: trainB* under --dataset_dir, or --dataset_dir_B")
        cache_B = D.DatasetCache(root_B, split_B, device=dev, max_files=args.train_size)
    batches = D.DirectoryBatches(model, args, cache_A, cache_B, augment=augment)
    tests = None
    if os.path.isdir(os.path.join(root, "testA")):
        cache = class_test_cache(args, root, dev, with_class=bool(getattr(args, "crf", False)))
        tests = D.directory_test_samples(args, cache)
        set_swd_reals(args, dev, len(cache))
    return batches, tests


def check_swd(args):
    """--swd: the test size must give at least one pyramid level."""
    from .kernels import swd_default_levels
    if getattr(args, "swd", False) and swd_default_levels(args.image_height, args.image_width) == 0:
        raise ValueError(f"--swd: {args.image_height}x{args.image_width} gives no pyramid level: the count is the largest L <= 5 for which "
                         "--img_height and --img_width divide by 2^(L-1) and min(H, W) >> (L-1) >= 16 (a coarsest level under 7x7 "
                         "could not hold one patch)")
    if getattr(args, "swd_patches", 128) <= 0:
        raise ValueError("--swd_patches must be positive")


def set_swd_reals(args, device, count):
    """--swd with --cycle on a dataset directory: ``args.swd_reals`` yields the first ``count`` images, in sorted order, of testB
    (else trainB) of the domain-B root (--dataset_dir_B, else --dataset_dir), resampled to the test size like the test samples.
    In every other case it stays unset and the reals are the test samples' label images."""
    from . import data as D
    if not (getattr(args, "swd", False) and args.cycle):
        return
    for split in ("testB", "trainB"):
        root_B = D.resolve_root(args.dataset_dir_B or args.dataset_dir, split)
        if root_B is not None:
            args.swd_reals = D.directory_images(args, root_B, split, count, device)
            return


def class_test_cache(args, root, device, with_class=False):
    """The testA cache; with --class_scores it holds the class maps and ``args.class_palette`` is learned from it."""
    from . import data as D
    if not getattr(args, "class_scores", False):
        return D.DatasetCache(root, "testA", device=device, with_class=with_class)
    folder = os.path.join(root, "testA_seg_class")
    if not os.path.isdir(folder):
        raise FileNotFoundError(f"--class_scores needs the class maps of the test set: {folder} does not exist")
    from .segment_class import learn_palette
    cache = D.DatasetCache(root, "testA", device=device, with_class=True)
    args.class_palette = learn_palette(cache)
    check_class_palette(args)
    return cache


def check_class_palette(args):
    """--class_scores: every palette class must be a class of the score (--segment_class)."""
    pal = getattr(args, "class_palette", None)
    if pal is not None and len(pal[1]) and int(max(pal[1])) >= args.segment_class:
        raise ValueError(f"--class_scores: the palette holds class {int(max(pal[1]))} but --segment_class is {args.segment_class}")


def main(argv=None):
    """main.py:45-60: ``--phase train`` runs the epoch loop (with the epoch-end test pass and scalar summaries of
    model.py:263-268), ``--phase test`` the test pass of model.py:535-567 -- on the dataset directory ``--dataset_dir``
    names, or on synthetic data where it names none."""
    args = parse_args(argv)
    check_swd(args)
    from . import data as D
    from .model import sggan
    from .utils import SummarySink
    model = sggan(args)
    if D.resolve_root(args.dataset_dir) or D.resolve_root(args.dataset_dir, "testA"):
        # a dataset given as a path: checkpoints go under <checkpoint_dir>/<its folder name>, as they do for a bare name
        model.dataset_dir = os.path.basename(os.path.normpath(args.dataset_dir)) or args.dataset_dir
    if args.phase == "test":          # main.py:58-60
        root = D.resolve_root(args.dataset_dir, "testA")
        if root is not None:
            cache = class_test_cache(args, root, model.device)
            set_swd_reals(args, model.device, len(cache))
            return model.test(args, D.directory_test_samples(args, cache)())
        return model.test(args, synthetic_test_samples(args)())
    sink = SummarySink(os.path.join(getattr(args, "log_dir", "./logs"), "train", "scalars.jsonl"))
    src = directory_sources(model, args)
    if src is not None:
        return model.train(args, src[0], test_samples=src[1], sink=sink)
    if getattr(args, "class_scores", False):          # synthetic samples: the built-in colour table
        from .segment_class import palette
        args.class_palette = palette()
        check_class_palette(args)
    if getattr(args, "augment", False):
        print(" [*] --augment has no effect on the synthetic batches (--dataset_dir names no folder with trainA)")
    return model.train(args, synthetic_batches(model, args), test_samples=synthetic_test_samples(args), sink=sink)


if __name__ == "__main__":
    main()
