"""CPU-side checks of the linear learning-rate decay (--lr_decay): the host statement of the rule
(kernels.scheduled_lr), the C ABI of sgg_adam_sched, the build resources of csrc/adam.hip and csrc/misc.hip and the flag."""
import os
import re

import numpy as np
import pytest

from sggan_amd import _abi as A
from tests.kernel_resources import kernel_resource_usage, the_kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_rule(lr, epoch, epoch_step, epochs):
    """model.py:223 as the reference writes it, in Python floats (``args.epoch`` is the epoch count there)."""
    return lr if epoch < epoch_step else lr * (epochs - epoch) / (epochs - epoch_step)


def test_scheduled_lr_known_answers():
    """lr 2e-4, epoch_step 2, epochs 5, 3 steps per epoch: flat for iterations 0-5, then 3/3, 2/3, 1/3 of lr, then 0; and the
    reference's commented expression evaluated in Python floats and rounded once to f32 gives the same f32 at every iteration.
    (scheduled_lr takes lr as the f32 the kernel receives and evaluates the decayed rate in double from that; for these
    values that is the f32 the all-double expression rounds to.)"""
    from sggan_amd.kernels import scheduled_lr
    lr, spe, step, epochs = 2e-4, 3, 2, 5
    got = [scheduled_lr(lr, it, spe, step, epochs) for it in range(21)]
    assert all(isinstance(v, np.float32) for v in got)
    for it in range(0, 6):
        assert got[it] == np.float32(2e-4), it
    for it in range(6, 9):
        assert got[it] == np.float32(2e-4 * 3 / 3), it
    for it in range(9, 12):
        assert got[it] == np.float32(2e-4 * 2 / 3), it
    for it in range(12, 15):
        assert got[it] == np.float32(2e-4 * 1 / 3), it
    for it in range(15, 21):
        assert got[it] == np.float32(0.0), it
    assert scheduled_lr(lr, 10 ** 12, spe, step, epochs) == np.float32(0.0)
    for it in range(15):                                   # the reference's loop never reaches epoch >= epochs
        assert got[it] == np.float32(_reference_rule(lr, it // spe, step, epochs)), it
    # epochs == epoch_step (the reference's defaults, 100 / 100): the rule would divide by zero -- lr at every iteration
    for it in (0, 1, 299, 300, 301, 10 ** 6):
        assert scheduled_lr(lr, it, spe, 100, 100) == np.float32(lr)
        assert scheduled_lr(lr, it, spe, 5, 3) == np.float32(lr)          # epochs < epoch_step: never decays either
    assert scheduled_lr(lr, 7, 0, 1, 4) == scheduled_lr(lr, 7, 1, 1, 4)   # steps_per_epoch is clamped to >= 1


def test_sgg_adam_sched_is_exported_bound_and_validates_on_the_host():
    """The symbol is declared in include/sggan.h with the issue's signature, bound with matching ctypes, and a call with null
    pointers (or n < 0) returns SGG_EINVAL before any launch -- no GPU needed."""
    import ctypes as C
    src = open(os.path.join(ROOT, "include", "sggan.h")).read()
    decl = re.search(r"int sgg_adam_sched\((.*?)\);", src, flags=re.S)
    assert decl, "sgg_adam_sched not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["float* theta", "const float* g", "float* m", "float* v", "int64_t n", "int64_t* state", "const int64_t* sched",
                      "float lr", "float beta1", "float beta2", "float eps", "float grad_scale", "void* stream"]
    vp, f = C.c_void_p, C.c_float
    assert A.SIGNATURES["sgg_adam_sched"] == (C.c_int, [vp, vp, vp, vp, C.c_int64, vp, vp, f, f, f, f, f, vp])
    L = A.lib()
    assert L.sgg_adam_sched.argtypes == A.SIGNATURES["sgg_adam_sched"][1]
    assert L.sgg_adam_sched(None, None, None, None, 10, None, None, 1e-3, 0.5, 0.999, 1e-7, 1.0, None) == A.EINVAL
    buf = (C.c_int64 * 4)()                                 # host memory: only ever compared against NULL, never dereferenced
    p = C.cast(buf, C.c_void_p)
    assert L.sgg_adam_sched(p, p, p, p, 1, p, None, 1e-3, 0.5, 0.999, 1e-7, 1.0, None) == A.EINVAL     # sched missing
    assert L.sgg_adam_sched(p, p, p, p, 1, None, p, 1e-3, 0.5, 0.999, 1e-7, 1.0, None) == A.EINVAL     # state missing
    assert L.sgg_adam_sched(p, p, p, p, -1, p, p, 1e-3, 0.5, 0.999, 1e-7, 1.0, None) == A.EINVAL       # n < 0


def test_misc_kernels_do_not_spill_and_use_no_scratch(tmp_path):
    """csrc/adam.hip and csrc/misc.hip recompiled with -Rpass-analysis=kernel-resource-usage (tests/kernel_resources.py): the
    prep kernel and the scalar update kernel are in the build, each once, and they and every other kernel of the two files have
    zero VGPR / SGPR spills and no scratch."""
    adam, misc = kernel_resource_usage("adam.hip", tmp_path), kernel_resource_usage("misc.hip", tmp_path)
    for frag in ("adam_prep_kernel", "adam_kernel"):
        the_kernel(adam, frag)
    assert len(adam) == 5 and len(misc) >= 39, (sorted(adam), sorted(misc))      # every kernel of the files reported
    for k, v in {**adam, **misc}.items():
        assert (v["vspill"], v["sspill"], v["scratch"]) == (0, 0, 0), (k, v)


# parse_args([]) before --lr_decay existed
_DEFAULTS_BEFORE = {
    "L1_lambda": 10.0, "Lg_lambda": 5.0, "augment": False, "batch_size": 1, "beta1": 0.5, "checkpoint_blocks": False,
    "checkpoint_dir": "./checkpoint", "continue_train": False, "crf": False, "cycle": False, "dataset_dir": "city",
    "dataset_dir_B": None, "dtype": "bf16", "epoch": 100, "epoch_step": 100, "generator": "resnet", "graph": False,
    "image_height": 64, "image_width": 64, "input_nc": 3, "log_dir": "./logs", "lr": 0.0002, "max_size": 50, "ndf": 64, "ngf": 64,
    "output_nc": 3, "paired": None, "phase": "train", "print_freq": 5, "ratio_gan2seg": 10, "sample_dir": "./sample",
    "save_freq": 1000, "segment_class": 34, "steps_per_epoch": 4, "test_dir": "./test", "train_size": 100000000,
    "use_augmentation": True, "use_lsgan": True, "use_pix2pix": False, "use_pool": False, "use_resnet": True,
    "which_direction": "AtoB"}


def test_lr_decay_flag():
    from sggan_amd.main import build_parser, parse_args
    assert parse_args(["--lr_decay"]).lr_decay is True
    assert parse_args([]).lr_decay is False
    got = vars(parse_args([]))
    assert got == dict(_DEFAULTS_BEFORE, lr_decay=False)                   # the default namespace gains only that key
    assert parse_args(["--epoch_step", "7"]).epoch_step == 7               # still parsed as it was
    text = " ".join(build_parser().format_help().split())
    for word in ("--lr_decay", "lr if epoch < epoch_step else", "--epoch_step", "--epoch", "--lr"):
        assert word in text, word


def test_default_model_arguments_leave_the_decay_off():
    from sggan_amd.model import default_args
    assert default_args().lr_decay is False and default_args(lr_decay=True).lr_decay is True
