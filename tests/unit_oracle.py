"""Float64 statement of ONE layer unit of module.py (conv -> (mask) -> instance norm -> record, and its backward), the derived
error bounds that go with it, and the table of cases at which the units' launch choices flip -- TEST INFRASTRUCTURE ONLY.

The comparison is teacher-forced and per unit: tests/unit_spy.py records what every ``_Unit.forward`` / ``_Unit.backward`` call
of a real walk was handed and what it returned; each call is compared here with the float64 result of that one layer on the
tensors the device itself stored, so no error is carried from layer to layer.  Built on oracle/sggan_oracle.py (conv2d,
deconv2d and their tape), tests/instnorm_oracle.py (the instance norm, its bounds, ``to_storage``, ``ulp``) and
tests/dropout_oracle.py (the masks).  Weights are the network's f32 parameters rounded to the storage type, as the pack launch
rounds them; bias, gamma and beta stay f32.

Stages of a forward call:  ``xc`` (the conv output; the masked and rescaled value at a dropout site; the activated value in a
layer without a norm), ``stats`` ((mean, rstd) of the STORED xc), ``y`` (act(IN(stored xc) + residual), or the skip form).
Stages of a backward call, from the recorded dy in the dtype the walk handed it: ``dx`` (with the addend), ``dskip``, ``partial``
(the next norm's backward sums against the returned dx) and per call the reference parts of ``dW``, ``db``, ``dgamma``,
``dbeta``, which check_param_grads compares with what the gradient buffers hold after the pass.

The bounds (nothing here is fitted to a device result):
  * one rounding to the storage type is half a unit in the last place of that type at the rounded value (instnorm_oracle.ulp):
    between 2^-9 and 2^-8 of the value for bfloat16 (8 significant bits), at most 2^-24 of it for float32;
  * an f32 accumulation of T terms in ANY order is within T * 2^-24 * (the sum of the absolute terms): T = R*S*C + 1 for the
    forward, R*S*K for the data gradient, N*Ho*Wo for the weight and bias gradients (each with a cotangent of its own in the
    pass that makes the sums of absolute terms);
  * the instance norm's own bounds of tests/instnorm_oracle.py (SAFETY included), with ``rel`` the larger of the norm's own chunk
    length and the conv epilogue's (HW / stats_chunks pixels) times 2^-24;
  * inside a backward call the gradient with respect to the conv output is a stored tensor the recorder does not see: its bound
    (norm backward, mask, rounding) is carried through sum |w| and sum |x| into the bounds of dx, dW and db;
  * a second storage rounding is granted only where include/sggan.h documents one: a transposed layer with an addend (a pass
    of its own), and a bf16 REFLECT data gradient without addend on the HALO_NARROW_IN / HALO_DGRAD_NARROW routes, on the rows
    and columns 1..p, H-1-p..H-2, W-1-p..W-2 that the mirrored terms reach, the first rounding at the zero-padded value;
  * tanh (ocml, f32) is taken to be within TANH_ULPS units in the last place of f32.
Activation kinks (backward only: every activation is 1-Lipschitz, so the forward needs none): where the reference's
pre-activation lies within the backward's own bound on it (backward_bounds' ``bpre``), either slope is accepted and |dy| times
the slopes' difference enters the bounds of everything that element reaches; at most KINK_FRACTION of a tensor may be so.  A
skip unit and a layer without a norm take the slope from the STORED output, as the kernels do: no ambiguity.  (Stage.kinks is
the fraction of the tensor's elements that were given either slope.)"""
from collections import namedtuple

import numpy as np

from oracle import sggan_oracle as O
from tests import dropout_oracle as D
from tests import instnorm_oracle as I

F64 = np.float64
U32 = 2.0 ** -24
TANH_ULPS = 4.0
KINK_FRACTION = 1e-4
NONE, RELU, LRELU, TANH = I.NONE, I.RELU, I.LRELU, I.TANH
EPS = 1e-3
FOLD_ROUTES = ("HALO_NARROW_IN", "HALO_DGRAD_NARROW")       # the data-gradient routes whose border fold is a launch of its own

Layer = namedtuple("Layer", "name kind stride padding reflect norm act leak R cin cout skip_grad drop_layer")


def cpad(c):
    return (c + 7) // 8 * 8


# ---------------------------------------------------------------------------- topologies (module.py, restated without a device)
def topology(net, width, n_blocks=2, in_c=3, out_c=3, classes=34, d_leak=0.3):
    """The layers of Generator / Discriminator / GeneratorUNet in conv_units() order."""
    L = lambda name, kind, cin, cout, stride=1, padding="VALID", reflect=0, norm=True, act=NONE, leak=0.0, R=3, skip=False, drop=None: \
        Layer(name, kind, stride, padding, reflect, norm, act, leak, R, cin, cout, skip, drop)
    w = width
    if net == "resnet":
        out = [L("c1", "conv", in_c, w, reflect=3, act=RELU, R=7), L("c2", "conv", w, 2 * w, 2, "SAME", act=RELU),
               L("c3", "conv", 2 * w, 4 * w, 2, "SAME", act=RELU)]
        for i in range(1, n_blocks + 1):
            out += [L(f"r{i}a", "conv", 4 * w, 4 * w, reflect=1, act=RELU), L(f"r{i}b", "conv", 4 * w, 4 * w, reflect=1)]
        return out + [L("d1", "deconv", 4 * w, 2 * w, 2, act=RELU), L("d2", "deconv", 2 * w, w, 2, act=RELU),
                      L("out", "conv", w, out_c, reflect=3, norm=False, act=TANH, R=7)]
    if net == "disc":
        D_ = lambda name, cin, cout, s, p, norm=True, act=LRELU: L(name, "conv", cin, cout, s, p, norm=norm, act=act, leak=d_leak if act == LRELU else 0.0)
        return [D_("h0", in_c, w, 2, "SAME", norm=False), D_("h1", w, 2 * w, 2, "SAME"), D_("h2", 2 * w, 4 * w, 2, "SAME"),
                D_("h3", 4 * w, 8 * w, 1, "SAME"), D_("h31", 8 * w, 8 * w, 2, "VALID"), D_("h32", 8 * w, 8 * w, 2, "VALID"),
                D_("h33", 8 * w, 8 * w, 1, "VALID"), D_("h4", 8 * w, classes, 1, "SAME", norm=False, act=NONE)]
    if net == "unet":
        enc = [in_c, w, 2 * w, 4 * w] + [8 * w] * 5
        out = [L(f"e{i}", "conv", enc[i - 1], enc[i], 1, "SAME", act=LRELU if i < 8 else RELU, leak=0.3 if i < 8 else 0.0) for i in range(1, 9)]
        dec = [8 * w] * 5 + [4 * w, 2 * w, w]
        for i in range(1, 8):
            out.append(L(f"d{i}", "deconv", dec[i - 1], dec[i], 1, "SAME", act=RELU if i in (3, 7) else NONE, skip=i in (3, 7),
                         drop=i - 1 if i <= 3 else None))
        return out + [L("d8", "deconv", w, out_c, 1, "SAME", norm=False, act=TANH)]
    raise ValueError(net)


def layer_of(u):
    """The Layer of a module.py unit (_ConvUnit or _PairUnit)."""
    return Layer(u.name, u.kind, u.stride, u.padding, u.reflect, bool(u.norm), int(u.act), float(u.leak), u.R, u.cin, u.cout,
                 bool(u.skip_grad), u.drop_layer)


def out_hw(L, H, W):
    if L.kind == "deconv":
        return H * L.stride, W * L.stride
    if L.reflect:
        return H + 2 * L.reflect - L.R + 1, W + 2 * L.reflect - L.R + 1
    if L.padding == "SAME":
        return -(-H // L.stride), -(-W // L.stride)
    return (H - L.R) // L.stride + 1, (W - L.R) // L.stride + 1


def plan(K, row, N=None):
    """{layer name: ConvGeom} of a row through the library's query functions (K = the package's ``kernels``; no GPU needed).
    N: the images of one launch (default: the row's batch, one network's share)."""
    import torch
    dt = {"bf16": torch.bfloat16, "f32": torch.float32}[row["dtype"]]
    N = row["batch"] if N is None else N
    H, W = row["image"]
    out = {}
    for L in topology(row["net"], row["width"], row.get("n_blocks", 2)):
        if L.kind == "conv":
            out[L.name] = K.conv_geom(N, H, W, cpad(L.cin), cpad(L.cout), L.R, L.R, L.stride, L.padding, L.reflect, dt)
        else:
            out[L.name] = K.deconv_geom(N, H, W, cpad(L.cin), cpad(L.cout), L.R, L.R, L.stride, dt)
        H, W = out_hw(L, H, W)
    return out


def describe(A, g):
    """The fields of a ConvGeom the case table names."""
    return dict(fwd=A.route_name(g.route_fwd), dgrad=A.route_name(g.route_dgrad), wgrad=A.route_name(g.route_wgrad), stats=g.stats_chunks,
                bwd_stats=g.bwd_stats_chunks, pair=bool(g.pair_ok), wgrad_pair=bool(g.wgrad_pair), mixed=bool(g.dgrad_mixed),
                normload=bool(g.normload_ok))


# ---------------------------------------------------------------------------- the case table
# Every row: network, width, dtype, image, batch (per network), pair (the lockstep form on the stacked batch of 2 * batch),
# switches (attributes set on the network(s)), dropout (U-Net), and
#   expect:   {layer: {field: value}} -- what the query functions must say (tests/test_unit_oracle_cpu.py asserts it without a GPU;
#             "r" stands for every residual 3x3 layer, "e4..e8" for those encoder layers);
#   launches: (symbols the run must call, symbols it must not call) -- the GPU test greps the recorded calls for them.
GENERIC = "GLDS_128x128+SPLITK"
_HALO_R = dict(fwd="HALO3", dgrad="HALO3", wgrad="W9", pair=True, wgrad_pair=True, mixed=True, normload=True)
_GEN_R = dict(fwd=GENERIC, dgrad=GENERIC, stats=0, bwd_stats=0, pair=False, wgrad_pair=False, mixed=False, normload=False)
_STEM = lambda n: dict(c1=dict(fwd="HALO_NARROW_IN", stats=n), out=dict(dgrad="HALO_NARROW_IN"))
_NOSTEM = dict(c1=dict(fwd="GLDS_128x64", stats=0), out=dict(dgrad="GLDS_128x64"))
_FS, _FSP = "sgg_conv2d_fwd_stats", "sgg_conv2d_fwd_stats_pair"

RESNET_IMAGES = {
    # image: (expectations, why)
    (16, 512): dict(_STEM(16), c2=dict(dgrad="S2HALO", wgrad="W9S"), c3=dict(dgrad=GENERIC), r=dict(_HALO_R, stats=4, bwd_stats=4),
                    d1=dict(fwd=GENERIC, stats=0), d2=dict(fwd="S2HALO", stats=8)),
    (24, 512): dict(_NOSTEM, c2=dict(dgrad="GLDS_128x64"), c3=dict(dgrad=GENERIC), r=dict(_HALO_R, stats=6, bwd_stats=6),
                    d1=dict(fwd=GENERIC, stats=0), d2=dict(fwd="GLDS_128x64", stats=0)),
    (20, 512): dict(_NOSTEM, c2=dict(dgrad="GLDS_128x64"), r=dict(_GEN_R, wgrad="WGRAD_V2_ROWFAST"), d1=dict(fwd=GENERIC), d2=dict(fwd="GLDS_128x64", stats=0)),
    (16, 384): dict(_STEM(12), c2=dict(dgrad="S2HALO"), c3=dict(dgrad=GENERIC), r=dict(_GEN_R, wgrad="WGRAD_V2"), d1=dict(fwd=GENERIC, stats=0),
                    d2=dict(fwd="S2HALO", stats=6)),
    (16, 256): dict(_STEM(8), c2=dict(dgrad="S2HALO"), c3=dict(dgrad=GENERIC), r=dict(_GEN_R, wgrad="W9", wgrad_pair=True),
                    d1=dict(fwd=GENERIC), d2=dict(fwd="S2HALO", stats=4)),
    (16, 192): dict(_STEM(6), c2=dict(dgrad="S2HALO", wgrad="WGRAD_128x128"), r=dict(_GEN_R, wgrad="WGRAD_V2"), d1=dict(fwd=GENERIC),
                    d2=dict(fwd="S2HALO", stats=3)),
    (16, 160): dict(_STEM(5), c2=dict(dgrad="GLDS_128x64"), r=dict(_GEN_R, wgrad="WGRAD_V2"), d1=dict(fwd=GENERIC), d2=dict(fwd="GLDS_128x64", stats=0)),
    (20, 132): dict(_NOSTEM, c2=dict(dgrad="GLDS_128x64"), r=dict(_GEN_R, wgrad="WGRAD_V2"), d1=dict(fwd=GENERIC), d2=dict(fwd="GLDS_128x64", stats=0)),
    # the smallest height (a multiple of 4) at which d1's forward and c3's data gradient take S2HALO at width 512 (the CPU test
    # searches the heights below it)
    (32, 512): dict(c3=dict(dgrad="S2HALO"), d1=dict(fwd="S2HALO", stats=4), d2=dict(fwd="S2HALO", stats=16), r=dict(_HALO_R, stats=8, bwd_stats=8)),
}
S2HALO_MIN_HEIGHT = 32
FUSED_R = {(16, 512), (24, 512), (32, 512)}          # images whose residual layers have the statistics epilogue


def _resnet_rows():
    rows = []

    def add(image, pair, tag="", switches=None, expect=None, launches=((), ()), **kw):
        base = dict(net="resnet", width=64, dtype="bf16", image=image, batch=2, pair=pair, switches=switches or {}, n_blocks=2,
                    expect=RESNET_IMAGES[image] if expect is None else expect, launches=launches)
        base.update(kw)
        base["id"] = f"resnet{base['width']}-{base['dtype']}-{image[0]}x{image[1]}-{'pair' if pair else 'single'}{'-' + tag if tag else ''}"
        rows.append(base)

    for image in RESNET_IMAGES:
        fused = image in FUSED_R
        add(image, False, launches=((_FS,), ()) if fused else ((), (_FS, _FSP)))
        add(image, True, launches=((_FSP, "sgg_conv2d_bwd_data_pair"), ()) if fused else ((), (_FS, _FSP, "sgg_conv2d_bwd_data_pair")))
    for image in ((16, 512), (20, 132)):
        fused = image in FUSED_R
        add(image, False, "mixed", dict(mixed=True), launches=(("sgg_conv2d_bwd_data_mixed",), ()) if fused else ((), ("sgg_conv2d_bwd_data_mixed",)))
        add(image, False, "fuse_in_bwd", dict(fuse_in_bwd=True),
            launches=(("sgg_conv2d_bwd_data_stats",), ()) if fused else ((), ("sgg_conv2d_bwd_data_stats",)))
        add(image, False, "no_fuse_in_stats", dict(fuse_in_stats=False), launches=((), (_FS, "sgg_deconv2d_fwd_stats")))
        # the pair without the statistics epilogue: the grouped forward on the 3x3 layers, the one-launch paired data gradient behind it
        add(image, True, "no_fuse_in_stats", dict(fuse_in_stats=False),
            launches=(("sgg_conv2d_fwd_group2",) + (("sgg_conv2d_bwd_data_pair",) if fused else ()),
                      (_FS, _FSP, "sgg_deconv2d_fwd_stats") + (() if fused else ("sgg_conv2d_bwd_data_pair",))))
        for pair in (False, True):
            add(image, pair, "stem_deconv_stats", dict(fuse_in_stats_stem=True, fuse_in_stats_deconv=True),
                launches=(("sgg_deconv2d_fwd_stats", _FS), ()) if fused else ((), ("sgg_deconv2d_fwd_stats",)))
            add(image, pair, "checkpoint", dict(checkpoint_blocks=True), launches=(((_FSP if pair else _FS),), ()) if fused else ((), ()))
        add(image, True, "no_group2", dict(group2=False), launches=((), ("sgg_conv2d_fwd_group2", "sgg_conv2d_bwd_weight_group2", "sgg_conv2d_bwd_data_group2")))
        # two applications of one network before the flush: the deferred weight-gradient pair; "other_shape": the second
        # application on an image two rows taller of the same route class -- the two-single-calls fallback
        add(image, False, "pair_wgrads", dict(pair_wgrads=True), applications=2,
            launches=(("sgg_conv2d_bwd_weight_pair",), ()) if fused else ((), ("sgg_conv2d_bwd_weight_pair",)))
    # a weight-gradient pair without a forward pair: W9 and wgrad_pair on layers whose forward and data gradient are generic
    add((16, 256), False, "pair_wgrads", dict(pair_wgrads=True), applications=2, launches=(("sgg_conv2d_bwd_weight_pair",), (_FS, _FSP)))
    add((16, 512), False, "pair_wgrads_other_shape", dict(pair_wgrads=True), applications=2, second_image=(24, 512),
        launches=((), ("sgg_conv2d_bwd_weight_pair",)))
    add((20, 132), False, "f32", dtype="f32", launches=((), (_FS,)),
        expect=dict(c1=dict(fwd="GLDS_128x64", stats=0), r=dict(_GEN_R, wgrad="WGRAD_V2"), out=dict(fwd="GLDS_256x16+SPLITK")))
    add((24, 512), False, "ngf32", width=32, launches=((_FS,), ()),
        expect=dict(c1=dict(fwd="GLDS_128x64", stats=0), c3=dict(wgrad="W9S"), r=dict(_HALO_R, stats=6, bwd_stats=6), d1=dict(fwd="GLDS_128x64", wgrad="W9S")))
    return rows


def _disc_rows():
    rows = []
    for dtype in ("bf16", "f32"):
        for image, exp in (((128, 128), dict(h1=dict(dgrad="S2HALO" if dtype == "bf16" else "GLDS_128x64+SPLITK"), h33=dict(fwd=GENERIC))),
                           ((116, 132), dict(h1=dict(dgrad="GLDS_128x64" if dtype == "bf16" else "GLDS_128x64+SPLITK"), h32=dict(fwd=GENERIC)))):
            for pair in (False, True):
                rows.append(dict(id=f"disc64-{dtype}-{image[0]}x{image[1]}-{'pair' if pair else 'single'}", net="disc", width=64, dtype=dtype,
                                 image=image, batch=1, pair=pair, switches={}, expect=exp,
                                 launches=(("sgg_conv2d_fwd_group2",), ()) if pair else ((), ("sgg_conv2d_fwd_group2",))))
    # At the two sizes above h33's map is one pixel: its instance norm returns beta, and every gradient in front of it is
    # identically zero -- device and reference agree at exactly 0, which pins nothing of the data gradients.  Two more sizes keep
    # the backward alive: 180x196 (maps 90x98, 45x49, 23x25, 11x12, 5x5, 3x3: odd maps under stride 2, a VALID column dropped)
    # and 160x256, where h1's data gradient takes S2HALO with a gradient that is not zero.
    for dtype, image, pair, exp in (("bf16", (180, 196), False, dict(h1=dict(dgrad="GLDS_128x64"), h33=dict(fwd=GENERIC))),
                                    ("bf16", (180, 196), True, dict(h1=dict(dgrad="GLDS_128x64"), h33=dict(fwd=GENERIC))),
                                    ("f32", (180, 196), False, dict(h1=dict(dgrad="GLDS_128x64+SPLITK"))),
                                    ("bf16", (160, 256), False, dict(h1=dict(dgrad="S2HALO"))), ("bf16", (160, 256), True, dict(h1=dict(dgrad="S2HALO")))):
        rows.append(dict(id=f"disc64-{dtype}-{image[0]}x{image[1]}-{'pair' if pair else 'single'}", net="disc", width=64, dtype=dtype,
                         image=image, batch=1, pair=pair, switches={}, expect=exp, live_backward=True,
                         launches=(("sgg_conv2d_fwd_group2",), ()) if pair else ((), ("sgg_conv2d_fwd_group2",))))
    return rows


DISC_MAPS_116x132 = ((58, 66), (29, 33), (15, 17), (15, 17), (7, 8), (3, 3), (1, 1), (1, 1))
_E_HALO = dict(fwd="HALO3", dgrad="HALO3", wgrad="W9", stats=128, pair=True, wgrad_pair=True)
_E_GEN = dict(stats=0, bwd_stats=0, pair=False, wgrad_pair=False, mixed=False)
UNET_IMAGES = {
    (128, 128): {"e4..e8": _E_HALO, "e3": dict(fwd="GLDS_128x64", dgrad="HALO3", stats=0), "d1": dict(fwd="HALO3", stats=0), "d7": dict(fwd="GLDS_256x16")},
    # e4..e8 off HALO3: the generic GEMM everywhere in the encoder's wide layers
    (32, 32): {"e4..e8": _E_GEN},
}


def _unet_rows():
    rows = []
    for image, exp in UNET_IMAGES.items():
        fused = image == (128, 128)
        for pair in (False, True):
            for dropout in (0.0, 0.5):
                fs = _FSP if pair else _FS
                row = dict(id=f"unet16-bf16-{image[0]}x{image[1]}-{'pair' if pair else 'single'}{'-dropout' if dropout else ''}", net="unet",
                           width=16, dtype="bf16", image=image, batch=1, pair=pair, switches={}, dropout=dropout, expect=exp,
                           launches=(((fs,) if fused else ()) + (("sgg_dropout",) if dropout else ()),
                                     (() if fused else (_FS, _FSP)) + (() if dropout else ("sgg_dropout",))))
                if pair and fused:
                    # the float64 reference of sixteen 128x128 layers is seconds per network: the lockstep run is made twice and
                    # each test holds one network's images and gradients to it
                    rows += [dict(row, id=row["id"] + "-net_" + "ab"[h], only_net=h) for h in (0, 1)]
                else:
                    rows.append(row)
    return rows


ROWS = _resnet_rows() + _disc_rows() + _unet_rows()
ROW_BY_ID = {r["id"]: r for r in ROWS}
assert len(ROW_BY_ID) == len(ROWS)


def expected_layers(row, key):
    """The layer names an ``expect`` key stands for."""
    names = [L.name for L in topology(row["net"], row["width"], row.get("n_blocks", 2))]
    if key == "r":
        return [n for n in names if n.startswith("r")]
    if key == "e4..e8":
        return [f"e{i}" for i in range(4, 9)]
    return [key]


# ---------------------------------------------------------------------------- one layer in float64
class Rec(namedtuple("Rec", "a name")):
    """A recorded device tensor: its values as a float32 array (exact for both storage types) and the storage type's name."""
    __slots__ = ()

    @property
    def f64(self):
        return self.a.astype(F64)


def _conv_tape(L, x, w, b):
    tape = O.Tape()
    vx, vw, vb = O.Var(x), O.Var(w), O.Var(b)
    if L.kind == "conv":
        y = O.conv2d(tape, vx, vw, vb, L.stride, L.padding, L.reflect)
    else:
        y = O.deconv2d(tape, vx, vw, vb, L.stride)
    return tape, vx, vw, vb, y


def _abs_conv(L, xa, wa, ba, cot=None):
    """The sums of absolute terms, which only enter bounds: the same layer on |x|, |w|, |b| in float32 torch (a second statement
    of the layer's geometry, held to the oracle's in tests/test_unit_oracle_cpu.py).  cot None: sum |x| |w| + |b|; else the
    vector-Jacobian products for two non-negative cotangents, ``cot`` = (the one for x, the one for w and b): the data gradient
    and the weight gradient accumulate different numbers of terms, so each gets its own.  Sums of non-negative float32 terms are
    within T * 2^-24 of their value: the results are scaled up by that."""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    x = t(xa).permute(0, 3, 1, 2).requires_grad_(cot is not None)
    w = t(wa).permute(3, 2, 0, 1).contiguous().requires_grad_(cot is not None)
    b = t(ba).requires_grad_(cot is not None)
    N, _, H, W = x.shape
    with torch.set_grad_enabled(cot is not None):
        if L.kind == "deconv":                            # the oracle's definition: the full scatter, cut at the SAME pads
            pt, pl = O.same_pads(H * L.stride, L.R, L.stride)[0], O.same_pads(W * L.stride, L.R, L.stride)[0]
            y = F.conv_transpose2d(x, w, b, stride=L.stride)[:, :, pt:pt + H * L.stride, pl:pl + W * L.stride]
        else:
            if L.reflect:
                xp = F.pad(x, (L.reflect,) * 4, mode="reflect")
            elif L.padding == "SAME":
                (pt, pb, _), (pl, pr, _) = O.same_pads(H, L.R, L.stride), O.same_pads(W, L.R, L.stride)
                xp = F.pad(x, (pl, pr, pt, pb))
            else:
                xp = x
            y = F.conv2d(xp, w, b, stride=L.stride)
    terms = max(L.R * L.R * max(L.cin, L.cout) + 1, y.shape[0] * y.shape[2] * y.shape[3])
    up = 1.0 + 2.0 * terms * U32
    if cot is None:
        return y.permute(0, 2, 3, 1).numpy().astype(F64) * up
    gx, = torch.autograd.grad(y, (x,), t(cot[0]).permute(0, 3, 1, 2), retain_graph=True)
    gw, gb = torch.autograd.grad(y, (w, b), t(cot[1]).permute(0, 3, 1, 2))
    return (gx.permute(0, 2, 3, 1).numpy().astype(F64) * up, gw.permute(2, 3, 1, 0).numpy().astype(F64) * up, gb.numpy().astype(F64) * up)


def conv_forward(L, x, w, b):
    """(conv(x), sum |x| |w| + |b|); the float64 convolution image by image (the im2col of a 7x7 layer is the large one).
    x: (N,H,W,cin) float64."""
    ys = [_conv_tape(L, x[n:n + 1], w, b)[4].v for n in range(x.shape[0])]
    return np.concatenate(ys), _abs_conv(L, np.abs(x), np.abs(w), np.abs(b))


def conv_backward(L, x, w, b, dxc, bdxc):
    """Gradients of conv(x) for the cotangent dxc, and their bounds for a cotangent known to within bdxc and f32 accumulation in
    any order -- R*S*K terms per element of dx, N*Ho*Wo per element of dw and db: dict(dx, dw, db, bdx, bdw, bdb) -- dx per image,
    dw / db summed over the images (before any storage rounding)."""
    N, Ho, Wo = dxc.shape[:3]
    Tx, Tw = L.R * L.R * L.cout, N * Ho * Wo
    dx = []
    dw = db = 0.0
    for n in range(N):
        tape, vx, vw, vb, y = _conv_tape(L, x[n:n + 1], w, b)
        tape.backward([(y, dxc[n:n + 1])])
        dx.append(vx.g)
        dw, db = dw + vw.g, db + vb.g
    bdx, bdw, bdb = _abs_conv(L, np.abs(x), np.abs(w), np.abs(b), (bdxc + Tx * U32 * np.abs(dxc), bdxc + Tw * U32 * np.abs(dxc)))
    return dict(dx=np.concatenate(dx), dw=dw, db=db, bdx=bdx, bdw=bdw + U32 * np.abs(dw), bdb=bdb + U32 * np.abs(db))


def store_bound(v, b, name, times=1):
    """The bound after `times` roundings to the storage type of a value v known to within b: half a unit in the last place at
    the largest magnitude it can have, per rounding."""
    for _ in range(times):
        b = b + 0.5 * I.ulp(np.abs(v) + b, name)
    return b


def act_forward(pre, bpre, L):
    """(act(pre), its bound) for a fused activation computed in f32: 1-Lipschitz, plus the activation's own rounding."""
    if L.act == TANH:
        y = np.tanh(pre)
        return y, bpre + TANH_ULPS * U32 * np.maximum(np.abs(y), 2.0 ** -126)
    y = I.act_fwd(pre, L.act, L.leak)
    return y, bpre + (U32 * np.abs(y) if L.act == LRELU else 0.0)


def act_slope_from_output(y, L):
    """act'(pre) from the stored output, as K.act_bwd derives it."""
    if L.act == TANH:
        return 1.0 - y * y
    if L.act == RELU:
        return (y > 0).astype(F64)
    if L.act == LRELU:
        return np.where(y > 0, 1.0, I.f32(L.leak))
    return np.ones_like(y)


def drop_mask(drop, n, H, W, C):
    """drop = (stream id, sample offset, step, seed, rate) -> (n,H,W,C) bool keep mask and the f32 scale."""
    stream, offset, t, seed, rate = drop
    return D.layer_mask(t, seed, stream, offset, n, H, W, C, rate), float(D.scale(D.threshold(rate)))


def norm_rel(name, HW, chunks):
    """``rel`` of the instance-norm bounds: the norm's own chunked pass, or the conv epilogue's rows (HW / chunks pixels each,
    f32 in any order) where the geometry has them -- the larger, since either may have made the sums."""
    rel = I.sum_rel(name, I.chain_pixels(HW, True))
    return max(rel, -(-HW // chunks) * U32) if chunks else rel


Stage = namedtuple("Stage", "stage ratio index err bound ref got kinks")


def compare(stage, got, ref, bound, kinks=0):
    got, ref, bound = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(bound, F64) + np.zeros_like(np.asarray(ref, F64))
    assert got.shape == ref.shape, (stage, got.shape, ref.shape)
    if got.size == 0:
        return Stage(stage, 0.0, (), 0.0, 0.0, 0.0, 0.0, kinks)
    err = np.abs(got - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    ratio = np.where(err == 0, 0.0, np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.inf))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return Stage(stage, float(ratio[i]), tuple(int(k) for k in i), float(err[i]), float(bound[i]), float(ref[i]), float(got[i]), kinks)


def pad_is_zero(stage, a, c_real):
    """The padded channels of an internal tensor hold exactly 0."""
    pad = np.asarray(a)[..., c_real:]
    bad = np.argwhere(pad != 0)
    return Stage(stage + ".pad", np.inf if len(bad) else 0.0, tuple(int(k) for k in bad[0]) if len(bad) else (), float(np.abs(pad).max()) if pad.size else 0.0,
                 0.0, 0.0, 0.0, 0)


def quantised_params(P, name):
    """The network's parameters as the launches use them: kernels rounded to the storage type (the pack launch), the rest f32."""
    return {k: (I.to_storage(v, name) if k.endswith("_w") else np.asarray(v, np.float32).astype(F64)) for k, v in P.items()}


def check_forward(L, P, call, eps=EPS):
    """One network's images of one forward call -> [Stage].  call: dict(x, xc, stats, y, residual, record_only, drop, stats_chunks)
    of Rec / None; P: quantised_params."""
    x, xc = call["x"], call["xc"]
    name = xc.name
    w, b = P[L.name + "_w"], P[L.name + "_b"]
    ref, sabs = conv_forward(L, x.f64[..., :L.cin], w, b)
    bound = (L.R * L.R * L.cin + 1) * U32 * sabs
    out = []
    got = xc.f64
    N, H, W, _ = got.shape
    if not L.norm:
        ref, bound = act_forward(ref, bound, L)
    bound = store_bound(ref, bound, name)
    if call.get("drop") is not None:
        keep, s = drop_mask(call["drop"], N, H, W, L.cout)
        ref, bound = np.where(keep, ref * s, 0.0), np.where(keep, store_bound(ref * s, bound * s + U32 * np.abs(ref * s), name), 0.0)
        dropped = xc.a[..., :L.cout][~keep]
        out.append(Stage("xc.dropped", 0.0 if not (dropped != 0).any() and not np.signbit(dropped).any() else np.inf, (), 0.0, 0.0, 0.0, 0.0, 0))
    out += [compare("xc", got[..., :L.cout], ref, bound), pad_is_zero("xc", xc.a, L.cout)]
    if not L.norm:
        return out
    xs = got[..., :L.cout]
    gamma, beta = P[L.name + "_g"], P[L.name + "_beta"]
    rel = norm_rel(name, H * W, call.get("stats_chunks", 0))
    mean, rstd = I.stats(xs, eps)
    bm, br = I.stats_bounds(xs, eps, rel)
    st = call["stats"].f64
    out += [compare("mean", st[:, :L.cout, 0], mean, bm), compare("rstd", st[:, :L.cout, 1], rstd, br)]
    if call.get("record_only") and call["y"] is None:
        return out
    res = None if call.get("residual") is None else call["residual"].f64[..., :L.cout]
    kw = dict(skip=res) if L.skip_grad else dict(residual=res)
    yref = I.forward(xs, gamma, beta, eps, L.act, L.leak, **kw)[0]
    by = I.forward_bounds(xs, gamma, beta, eps, L.act, L.leak, name, rel, **kw)[0]
    out += [compare("y", call["y"].f64[..., :L.cout], yref, by), pad_is_zero("y", call["y"].a, L.cout)]
    return out


def check_backward(L, P, call, eps=EPS, refs=None):
    """One network's images of one backward call -> ([Stage], parts): parts = {key: (reference, bound)} of this call's share of
    dW / db / dgamma / dbeta (absent where the unit writes none).  call: dict(x, xc, stats, y, dy, addend, dx, dskip, partial,
    next, drop, param_grads, bwd_stats_chunks) of Rec / None; next = (Layer, xc, stats, gamma, beta) of the consuming norm.
    refs: a dict that receives the float64 references (dx, dskip) themselves (the finite-difference test reads them)."""
    x, xc, dy = call["x"], call["xc"], call["dy"]
    name = xc.name                                       # the storage type of the gradient with respect to the conv output
    w, b = P[L.name + "_w"], P[L.name + "_b"]
    xs, g = xc.f64[..., :L.cout], dy.f64[..., :L.cout]
    N, H, W, _ = xs.shape
    out, parts, kinks = [], {}, 0
    if L.norm:
        gamma, beta = P[L.name + "_g"], P[L.name + "_beta"]
        st = call["stats"].f64
        mean, rstd = st[:, :L.cout, 0], st[:, :L.cout, 1]
        rel = norm_rel(name, H * W, call.get("bwd_stats_chunks", 0))
        extra = np.zeros_like(g)
        if L.skip_grad:
            slope = act_slope_from_output(call["y"].f64[..., :L.cout], L)
        else:
            slope = I.slope(gamma * ((xs - mean[:, None, None, :]) * rstd[:, None, None, :]) + beta, L.act, L.leak)
        gs = g * slope
        o = I.backward(gs, xs, gamma, beta, mean, rstd, NONE, 0.0)
        bb = I.backward_bounds(gs, xs, gamma, beta, mean, rstd, NONE, 0.0, name, rel, store_g=L.skip_grad)
        if not L.skip_grad and L.act in (RELU, LRELU):
            amb = np.abs(o["pre"]) <= bb["bpre"]             # (bpre bounds the backward's own gamma * xhat + beta: it does not depend on g)
            kinks = float(amb.mean())
            extra = np.where(amb, np.abs(g) * (1.0 - (I.f32(L.leak) if L.act == LRELU else 0.0)), 0.0)
        xh, A = o["xhat"], np.abs(gamma * rstd[:, None, None, :])
        mean_ = lambda a: a.mean((1, 2), keepdims=True)
        dxc, bdxc = o["dx"], bb["dx"] + A * (extra + mean_(extra) + np.abs(xh) * mean_(extra * np.abs(xh)))
        if call["param_grads"]:
            parts["dgamma"] = (o["dgamma"], bb["dgamma"] + (extra * np.abs(xh)).sum((0, 1, 2)))
            parts["dbeta"] = (o["dbeta"], bb["dbeta"] + extra.sum((0, 1, 2)))
        if refs is not None:
            refs["dskip"] = o["dskip"]
        if L.skip_grad and call.get("dskip") is not None:
            out += [compare("dskip", call["dskip"].f64[..., :L.cout], o["dskip"], bb["dskip"]), pad_is_zero("dskip", call["dskip"].a, L.cout)]
        if call.get("drop") is not None:
            keep, s = drop_mask(call["drop"], N, H, W, L.cout)
            dxc, bdxc = np.where(keep, dxc * s, 0.0), np.where(keep, store_bound(dxc * s, bdxc * s + U32 * np.abs(dxc * s), name), 0.0)
    else:
        slope = act_slope_from_output(xs, L)
        gq = I.to_storage(g, name) if dy.name != name else g             # (dy.to(xc.dtype): one rounding, known exactly)
        dxc = gq * slope
        bdxc = store_bound(dxc, 3 * U32 * np.abs(dxc), name) if L.act != NONE else np.zeros_like(dxc)
    r = conv_backward(L, x.f64[..., :L.cin], w, b, dxc, bdxc)
    if call["param_grads"]:
        parts["dw"] = (r["dw"], r["bdw"])
        if call.get("drop") is not None or not L.norm:
            parts["db"] = (r["db"], r["bdb"])
    ref, bound, times = r["dx"], r["bdx"], 1
    if call.get("addend") is not None:
        ref = ref + call["addend"].f64[..., :L.cin]
        bound = bound + U32 * np.abs(ref)
        times += L.kind == "deconv"                                      # (a transposed layer adds in a pass of its own)
    if refs is not None:
        refs["dx"] = ref
    if call.get("dx") is not None:
        dx = call["dx"]
        full = store_bound(ref, bound, dx.name, times)
        if (L.reflect and dx.name == "bf16" and call.get("addend") is None and call.get("dgrad_route") in FOLD_ROUTES):
            # include/sggan.h: the main launch pads with zeros and stores bf16(dx_zero); the border fold adds the mirrored terms
            # and rounds again, on the rows and columns those terms reach.  The first rounding is at dx_zero's magnitude.
            zero = conv_backward(L._replace(reflect=0, padding="SAME"), x.f64[..., :L.cin], w, b, dxc, bdxc)["dx"]
            H_, W_, p_ = ref.shape[1], ref.shape[2], L.reflect
            rows = np.zeros(H_, bool); rows[1:p_ + 1] = True; rows[H_ - 1 - p_:H_ - 1] = True
            cols = np.zeros(W_, bool); cols[1:p_ + 1] = True; cols[W_ - 1 - p_:W_ - 1] = True
            band = (rows[:, None] | cols[None, :])[None, :, :, None]
            full = np.where(band, store_bound(ref, bound + 0.5 * I.ulp(np.abs(zero) + bound, dx.name), dx.name, 1), full)
        out += [compare("dx", dx.f64[..., :L.cin], ref, full, kinks), pad_is_zero("dx", dx.a, L.cin)]
        if call.get("partial") is not None:
            nL, nxc, nst, ngamma, nbeta = call["next"]
            rows = call["partial"].f64.sum(1)[:, :nL.cout]               # (the consumer adds the chunks: their partition is the kernel's own)
            nx, nstat, dxs = nxc.f64[..., :nL.cout], nst.f64[:, :nL.cout], dx.f64[..., :nL.cout]
            nrel = norm_rel(dx.name, nx.shape[1] * nx.shape[2], call["partial"].a.shape[1])
            s1, s2, b1, b2, namb = [], [], [], [], 0
            for n in range(nx.shape[0]):                                 # per image: the bounds of one image's totals
                a_ = (dxs[n:n + 1], nx[n:n + 1], ngamma, nbeta, nstat[n:n + 1, :, 0], nstat[n:n + 1, :, 1], nL.act, nL.leak)
                on, nb = I.backward(*a_), I.backward_bounds(*a_, dx.name, nrel)
                amb = np.abs(on["pre"]) <= nb["bpre"] if nL.act in (RELU, LRELU) else np.zeros(on["pre"].shape, bool)
                ex = np.where(amb, np.abs(dxs[n:n + 1]), 0.0)
                namb += int(amb.sum())
                s1.append(on["dbeta"]); s2.append(on["dgamma"])
                b1.append(nb["dbeta"] + ex.sum((0, 1, 2))); b2.append(nb["dgamma"] + (ex * np.abs(on["xhat"])).sum((0, 1, 2)))
            out += [compare("partial.g", rows[..., 0], np.stack(s1), np.stack(b1), namb / dxs.size),
                    compare("partial.gx", rows[..., 1], np.stack(s2), np.stack(b2), namb / dxs.size)]
    return out, parts


def check_param_grads(L, parts_list, grads, accumulations=1):
    """The gradient buffers after the pass against the sum of the calls' reference parts.  grads: {key: float array of the real
    shape}; every f32 accumulation onto the buffer adds 2^-24 of the magnitudes."""
    out = []
    for key in ("dw", "db", "dgamma", "dbeta"):
        have = [p[key] for p in parts_list if key in p]
        if not have:
            if key in grads and key in ("db",):       # a bias in front of an instance norm: its gradient is left at exactly 0
                out.append(Stage(key + ".zero", np.inf if np.any(np.asarray(grads[key]) != 0) else 0.0, (), 0.0, 0.0, 0.0, 0.0, 0))
            continue
        ref = sum(r for r, _ in have)
        bound = sum(b for _, b in have) + (len(have) + accumulations) * U32 * sum(np.abs(r) for r, _ in have)
        out.append(compare(key, grads[key], ref, bound))
    return out


def worst(stages):
    return max(stages, key=lambda s: s.ratio)


