"""The layer units of module.py (conv -> (mask) -> instance norm -> record, and its backward) against what they launched and
computed on the commit BEFORE their forward and backward were folded into one body: per configuration, every call that two
eager training steps make into the library, in order, and SHA-256 digests of what the steps left behind.

tests/golden/unit_trace.json holds both (tests/golden/make_unit_trace.py wrote it, with the functions of this module; the
library under test never regenerates it).  The parity tests compare the single and the lockstep sequencing with each other and
with float64, which says little once the two share their body, and none of them can see a change that computes the same bits
with other launches -- two per-network calls where one grouped call ran.  This one compares both with what they did before.

The trace is taken by a proxy put in place of the bound library (``_abi._lib``) for the duration of a run: one entry per call
-- symbol, the 14 descriptor fields of a conv-family call, every integer and float scalar, for every pointer only whether it
is NULL, and the status returned.  Query calls (``*_workspace``, ``*_chunks``, ``*_supported``, ``*_route``, version, strerror)
are left out.  The shared scratch workspace is dropped before a run, so the workspace sizes in the entries are those of a
fresh process whatever ran before.  The digests cover the raw bytes of every network's ``P.flat`` and ``P.m`` and of the two
losses after the second step; there is no tolerance.  Step inputs are a closed-form integer hash (test_gpu_adam_bits.py), no
library random generator.

Shapes: the smallest at which the units' geometry-dependent branches are live (the library's own query functions say so
without a GPU: K.conv_geom / K.deconv_geom).  The discriminator's two VALID stride-2 layers need at least 113 pixels a side, so
the height is 128 everywhere.  ResNet, bf16, ngf 64, 128 x 512: the stem has statistics chunks (HALO_NARROW_IN), the residual
3x3 layers run HALO3 / W9 with forward and backward statistics chunks, the mixed data gradient, paired weight gradients and,
on the stacked batch, the one-launch lockstep forms; d1 / d2 run S2HALO with statistics chunks (at 128 x 256 the residual
layers fall to the generic GEMM, at ngf 32 the stem and d2 do).  U-Net, bf16, ngf 16, 128 x 128: e4..e8 run HALO3 / W9 with
statistics chunks, paired weight gradients and the lockstep forms.  One f32 case, ngf 8, 128 x 128: the generic routes only."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_adam_bits import hashed_f32

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unit_trace.json")
STEPS = 2

RESNET = dict(use_resnet=True, dtype="bf16", ngf=64, ndf=8, n_blocks=2, image_height=128, image_width=512)
UNET = dict(use_resnet=False, dtype="bf16", ngf=16, ndf=8, image_height=128, image_width=128)
F32 = dict(use_resnet=True, dtype="f32", ngf=8, ndf=8, n_blocks=2, image_height=128, image_width=128)
STEM_DECONV = dict(fuse_in_stats_stem=True, fuse_in_stats_deconv=True)

# configuration -> keywords of default_args (batch 1 unless given)
CASES = {
    "resnet/ref": dict(RESNET),
    "resnet/ref_no_d_quad": dict(RESNET, d_quad=False),
    "resnet/ref_mixed": dict(RESNET, mixed=True),
    "resnet/ref_fuse_in_bwd": dict(RESNET, fuse_in_bwd=True),
    "resnet/ref_no_fuse_in_stats": dict(RESNET, fuse_in_stats=False),
    "resnet/ref_stem_deconv_stats": dict(RESNET, **STEM_DECONV),
    "resnet/ref_checkpoint": dict(RESNET, checkpoint_blocks=True),
    "resnet/cycle_unpaired": dict(RESNET, cycle=True, paired=False),
    "resnet/cycle_paired": dict(RESNET, cycle=True),
    "resnet/cycle_paired_no_d_quad_no_group2": dict(RESNET, cycle=True, d_quad=False, group2=False),
    "resnet/cycle_paired_stem_deconv_stats": dict(RESNET, cycle=True, **STEM_DECONV),
    "resnet/cycle_paired_checkpoint": dict(RESNET, cycle=True, checkpoint_blocks=True),
    "resnet/cycle_paired_spectral": dict(RESNET, cycle=True, d_norm="spectral"),
    "resnet/cycle_paired_batch2": dict(RESNET, cycle=True, batch_size=2),       # (stacked batches of 4: more than one image per network)
    "unet/ref_dropout": dict(UNET, dropout=0.5),
    "unet/cycle_unpaired_dropout": dict(UNET, cycle=True, paired=False, dropout=0.5),
    "unet/cycle_paired_dropout": dict(UNET, cycle=True, paired=True, dropout=0.5),
    "unet/cycle_paired": dict(UNET, cycle=True, paired=True),
    "f32/cycle_paired": dict(F32, cycle=True),
}

_QUERY_ENDINGS = ("_workspace", "_workspace_bytes", "_chunks", "_supported", "_route", "_elems")
_QUERY_NAMES = ("sgg_version", "sgg_strerror")


def is_query(name):
    return name in _QUERY_NAMES or name.endswith(_QUERY_ENDINGS)


def encode(signatures, desc_ptr, name, args, status):
    """One call -> [symbol, descriptor fields or None, scalars, NULL flags of the pointers ('1': NULL), status]."""
    desc, scalars, nulls = None, [], ""
    for t, a in zip(signatures[name][1], args):
        if t is desc_ptr:
            d = a._obj                                    # (the launchers pass byref(desc))
            desc = [int(getattr(d, f)) for f, _ in d._fields_]
        elif t is C.c_float:
            scalars.append(C.c_float(a).value)            # (the value the callee sees)
        elif t in (C.c_int, C.c_int64, C.c_size_t, C.c_uint32):
            scalars.append(int(getattr(a, "value", a)))
        else:                                             # a pointer: c_void_p / POINTER(...)
            nulls += "1" if a is None or not getattr(a, "value", a) else "0"
    return [name, desc, scalars, nulls, int(status)]


class TraceLib:
    """Stands where ``_abi._lib`` stands: every attribute is the bound library's, the launches wrapped to append their entry."""

    def __init__(self, abi, real):
        self._abi, self._real, self.entries = abi, real, []
        self._desc_ptr = C.POINTER(abi.ConvDesc)

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if is_query(name) or name not in self._abi.SIGNATURES:
            return fn

        def call(*args):
            status = fn(*args)
            self.entries.append(encode(self._abi.SIGNATURES, self._desc_ptr, name, args, status))
            return status
        self.__dict__[name] = call
        return call


def step_inputs(stream, n, H, W, mh, mw, classes):
    """(image, label image, one-hot mask) of one domain: images in [0, 1) from hashed_f32 streams, the mask's class per cell from a third."""
    img = lambda s: ((hashed_f32(s, n * H * W * 3) + np.float32(1)) * np.float32(0.5)).reshape(n, H, W, 3)
    idx = np.minimum(((hashed_f32(stream + 2, n * mh * mw) + np.float32(1)) * np.float32(0.5 * classes)).astype(np.int64), classes - 1)
    mask = np.zeros((n * mh * mw, classes), dtype=np.float32)
    mask[np.arange(idx.size), idx] = 1.0
    return img(stream), img(stream + 1), mask.reshape(n, mh, mw, classes)


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def run_case(sg, case):
    """STEPS eager training steps of ``case`` on a fresh model -> ([entries of step 1, entries of step 2], digests)."""
    A, K = sg._abi, sg.kernels
    kw = dict(CASES[case])
    n = kw.setdefault("batch_size", 1)
    m = sg.sggan(sg.default_args(**kw))
    H, W = m.image_height, m.image_width
    mh, mw = m.discriminator.out_hw(H, W)
    m.real_A, m.seg_A, m.mask_A = step_inputs(1, n, H, W, mh, mw, m.segment_class)
    if m.cycle:
        m.real_B, m.seg_B, m.mask_B = step_inputs(4, n, H, W, mh, mw, m.segment_class)
    torch.cuda.synchronize()
    K._WS.clear()                                         # (the scratch workspace grows with what ran before: start from none)
    real = A.lib()
    proxy = TraceLib(A, real)
    steps = []
    A._lib = proxy
    try:
        for _ in range(STEPS):
            start = len(proxy.entries)
            m.train_step()
            steps.append(proxy.entries[start:])
        torch.cuda.synchronize()
    finally:
        A._lib = real
    digests = {}
    for name, net in zip(m._net_names(), m.networks()):
        digests[name + ".flat"], digests[name + ".m"] = _sha(net.P.flat), _sha(net.P.m)
    digests["gen_loss"], digests["disc_loss"] = _sha(m.gen_loss), _sha(m.disc_loss)
    return steps, digests


def recorded_steps(recorded, case):
    """The fixture's entries of ``case``, per step (the fixture stores distinct entries and distinct step sequences once)."""
    return [[recorded["entries"][i] for i in recorded["sequences"][s]] for s in recorded["cases"][case]["steps"]]


def first_difference(case, got, want):
    """None, or a message naming the configuration, the step and position, the recorded entry and the entry found."""
    for step, (g, w) in enumerate(zip(got, want), 1):
        for pos in range(max(len(g), len(w))):
            a, b = (g[pos] if pos < len(g) else None), (w[pos] if pos < len(w) else None)
            if a != b:
                return f"{case}: step {step}, call {pos} of {len(w)} recorded ({len(g)} made):\n  recorded {b}\n  found    {a}"
    return None if len(got) == len(want) else f"{case}: {len(got)} steps run, {len(want)} recorded"


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    return sggan_amd


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", list(CASES))
def test_units_launch_and_compute_what_they_did_before(sg, recorded, case):
    steps, digests = run_case(sg, case)
    steps = json.loads(json.dumps(steps))                 # (as the fixture went through JSON)
    diff = first_difference(case, steps, recorded_steps(recorded, case))
    assert diff is None, diff
    want = recorded["cases"][case]["digests"]
    if want is not None:                                  # (None: the case did not repeat its bits on the recording commit)
        moved = [k for k in want if digests.get(k) != want[k]]
        assert set(digests) == set(want) and not moved, (case, moved)
