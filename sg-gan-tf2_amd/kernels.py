"""Tensor-level launchers over the C ABI (one function per entry point of include/sggan.h).

torch is used for device memory and streams only: every function passes raw device
pointers + the current HIP stream to libsggan.so.  Tensors are NHWC, channel-padded
to a multiple of 8 (see include/sggan.h), float32 (parity path) or bfloat16 (perf path).
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import torch

from . import _abi as A

_DT = {torch.float32: A.SGG_F32, torch.bfloat16: A.SGG_BF16}


def dt(t_or_dtype) -> int:
    d = t_or_dtype.dtype if isinstance(t_or_dtype, torch.Tensor) else t_or_dtype
    try:
        return _DT[d]
    except KeyError:
        raise TypeError(f"unsupported dtype {d}: activations must be float32 or bfloat16")


def cpad(c: int) -> int:
    return (c + A.CPAD - 1) // A.CPAD * A.CPAD


def _p(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensor required"
    return C.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device


def _s():
    """The current HIP stream of the current device as a raw handle.  torch.cuda.current_stream() builds a Stream
    object per call (~8 us, 750 launches per step); the raw accessor is one C call."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(_raw_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_WS = {}

# Optional timing hook (bench.py): PROFILE(op_name, geom_or_shape) -> object with start()/stop(), or None.
# Events are recorded on the current stream, i.e. the stream the kernel is launched on.
PROFILE = None


def _prof(name, key):
    return PROFILE(name, key) if PROFILE is not None else None


# Host-side actions in step order (graph.StepProgram.host): while a step is being recorded into HIP graphs the recorder is
# installed here; an action then ends the current graph segment and is replayed between segments.  Otherwise it just runs.
_RECORDER = None


def host(fn):
    return fn() if _RECORDER is None else _RECORDER.host(fn)



def workspace(nbytes: int, device) -> torch.Tensor:
    """Per-device scratch buffer shared by all launches (single stream => in-order reuse is safe)."""
    key = torch.device(device).index or 0
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = ws
    return ws


def workspace_refs():
    """The scratch buffers currently in use (a recorded StepProgram holds them: their addresses are in its launches)."""
    return list(_WS.values())


def same_pads(n_in: int, k: int, s: int):
    """TF 'SAME' (leading pad, trailing pad, output size): the extra pad goes bottom/right."""
    out = -(-n_in // s)
    total = max((out - 1) * s + k - n_in, 0)
    return total // 2, total - total // 2, out


class ConvGeom:
    """Geometry of one Conv2D / Conv2DTranspose call site, resolved to an sgg_conv_desc."""
    __slots__ = ("desc", "x_shape", "y_shape", "ws_wgrad", "ws_dgrad", "ws_fwd", "dtype", "is_deconv", "stats_chunks", "wgrad_pair", "bwd_stats_chunks", "dgrad_mixed", "pair_ok", "normload_ok",
                 "route_fwd", "route_dgrad", "route_wgrad")

    def __init__(self, desc, x_shape, y_shape, dtype, is_deconv):
        self.desc, self.x_shape, self.y_shape, self.dtype, self.is_deconv = desc, x_shape, y_shape, dtype, is_deconv
        self.ws_wgrad = int(A.lib().sgg_conv2d_bwd_weight_workspace(C.byref(desc)))
        L = A.lib()
        # pixel chunks of the (sum, sumsq) rows the forward conv can emit for a following instance norm (0: it cannot)
        self.stats_chunks = int((L.sgg_deconv2d_fwd_stats_chunks if is_deconv else L.sgg_conv2d_fwd_stats_chunks)(C.byref(desc)))
        # the weight gradients of two applications of the layer can share one launch (cycle step)
        self.wgrad_pair = (not is_deconv) and bool(L.sgg_conv2d_bwd_weight_pair_supported(C.byref(desc)))
        # chunks of the norm-backward partial sums the data gradient can emit for the norm that consumes dx (0: it cannot)
        self.bwd_stats_chunks = 0 if is_deconv else int(L.sgg_conv2d_bwd_data_stats_chunks(C.byref(desc)))
        # mixed mode: the data gradient can be written in f32 (bf16 operands) for the norm backward that consumes it
        self.dgrad_mixed = (not is_deconv) and bool(L.sgg_conv2d_bwd_data_mixed_supported(C.byref(desc)))
        # a stacked batch of two networks can run forward (+stats) / data gradient as ONE launch with per-image weights
        self.pair_ok = (not is_deconv) and bool(L.sgg_conv2d_pair_supported(C.byref(desc)))
        self.normload_ok = (not is_deconv) and bool(L.sgg_conv2d_fwd_normload_supported(C.byref(desc)))
        # workspaces of the two GEMM directions; a deconv runs the conv's data-gradient kernel forwards
        self.ws_fwd = int((L.sgg_deconv2d_fwd_workspace if is_deconv else L.sgg_conv2d_fwd_workspace)(C.byref(desc)))
        self.ws_dgrad = int((L.sgg_deconv2d_bwd_data_workspace if is_deconv else L.sgg_conv2d_bwd_data_workspace)(C.byref(desc)))
        # the kernel each plain call launches (A.route_name: 'HALO3', 'GLDS_128x128+SPLITK', ...), from the launchers' own selection code
        route = L.sgg_deconv2d_route if is_deconv else L.sgg_conv2d_route
        self.route_fwd, self.route_dgrad, self.route_wgrad = (int(route(C.byref(desc), op)) for op in (A.ROUTE_OP_FWD, A.ROUTE_OP_DGRAD, A.ROUTE_OP_WGRAD))
        if self.ws_wgrad == 0:
            raise A.SggError(f"invalid convolution geometry {[(f, getattr(desc, f)) for f, _ in desc._fields_]}")


@functools.lru_cache(maxsize=None)
def conv_geom(N, H, W, C_, K, R, S, stride, padding, reflect, dtype) -> ConvGeom:
    """tf.keras.layers.Conv2D geometry: padding 'SAME'|'VALID', or reflect=p (tf.pad REFLECT then VALID)."""
    if reflect:
        assert padding == "VALID" and stride == 1
        pt = pl = reflect
        Ho, Wo = H + 2 * reflect - R + 1, W + 2 * reflect - S + 1
        mode = A.PAD_REFLECT
    elif padding == "SAME":
        pt, _, Ho = same_pads(H, R, stride)
        pl, _, Wo = same_pads(W, S, stride)
        mode = A.PAD_ZERO
    elif padding == "VALID":
        pt = pl = 0
        Ho, Wo = (H - R) // stride + 1, (W - S) // stride + 1
        mode = A.PAD_ZERO
    else:
        raise ValueError(padding)
    if Ho <= 0 or Wo <= 0:
        raise ValueError(f"convolution output is empty for input {H}x{W}, kernel {R}x{S}, stride {stride}, {padding}")
    d = A.ConvDesc(N, H, W, C_, K, R, S, stride, pt, pl, Ho, Wo, mode, dt(dtype))
    return ConvGeom(d, (N, H, W, C_), (N, Ho, Wo, K), dtype, False)


@functools.lru_cache(maxsize=None)
def deconv_geom(N, Hin, Win, Cin, Cout, R, S, stride, dtype) -> ConvGeom:
    """Conv2DTranspose(padding='same'): described by the equivalent conv whose INPUT is the deconv OUTPUT."""
    H, W = Hin * stride, Win * stride
    pt, _, oh = same_pads(H, R, stride)
    pl, _, ow = same_pads(W, S, stride)
    assert oh == Hin and ow == Win
    d = A.ConvDesc(N, H, W, Cout, Cin, R, S, stride, pt, pl, Hin, Win, A.PAD_ZERO, dt(dtype))
    return ConvGeom(d, (N, Hin, Win, Cin), (N, H, W, Cout), dtype, True)


# ----------------------------------------------------------------------------- weights
def pack_weights(w_hwio: torch.Tensor, Cp: int, Kp: int, dtype, want_fwd=True, want_dgrad=True):
    R, S, Cr, Kr = w_hwio.shape
    assert w_hwio.dtype == torch.float32
    wf = torch.empty((Kp, R * S * Cp), dtype=dtype, device=w_hwio.device) if want_fwd else None
    wd = torch.empty((Cp, R * S * Kp), dtype=dtype, device=w_hwio.device) if want_dgrad else None
    A.check(A.lib().sgg_pack_conv_weights(_p(w_hwio), R, S, Cr, Kr, Cp, Kp, dt(dtype), _p(wf), _p(wd), _s()), "pack_conv_weights")
    return wf, wd


def pack_weights_batch(entries, dtype, device):
    """entries: [(w_hwio f32 view, Cp, Kp, want_fwd, want_dgrad)].  Allocates the packed buffers once and returns
    (table, n, max_elems, [(wf, wd)]): the device table of sgg_pack_item for repack_batch()."""
    items = (A.PackItem * len(entries))()
    bufs, max_elems = [], 0
    for it, (w, Cp, Kp, want_fwd, want_dgrad) in zip(items, entries):
        R, S, Cr, Kr = w.shape
        assert w.is_contiguous() and w.dtype == torch.float32
        wf = torch.empty((Kp, R * S * Cp), dtype=dtype, device=device) if want_fwd else None
        wd = torch.empty((Cp, R * S * Kp), dtype=dtype, device=device) if want_dgrad else None
        it.w, it.w_fwd, it.w_dgrad = w.data_ptr(), (wf.data_ptr() if wf is not None else None), (wd.data_ptr() if wd is not None else None)
        it.taps, it.C, it.K, it.Cpad, it.Kpad, it.reserved = R * S, Cr, Kr, Cp, Kp, 0
        bufs.append((wf, wd))
        max_elems = max(max_elems, R * S * Cp * Kp)
    raw = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(device)
    return raw, len(entries), max_elems, bufs


def repack_batch(table, n, max_elems, dtype, scale=None):
    """scale: a device f32 vector, one factor per item, multiplied in f32 before the rounding (``sgg_pack_conv_weights_batch_scaled``)."""
    if scale is None:
        A.check(A.lib().sgg_pack_conv_weights_batch(_p(table), n, max_elems, dt(dtype), _s()), "pack_conv_weights_batch")
    else:
        assert scale.dtype == torch.float32 and scale.numel() == n
        A.check(A.lib().sgg_pack_conv_weights_batch_scaled(_p(table), _p(scale), n, max_elems, dt(dtype), _s()), "pack_conv_weights_batch_scaled")


# ----------------------------------------------------------------------------- conv / deconv
def _out(out, shape, dtype, device):
    """The caller's output buffer (a contiguous slice of a stacked pair tensor) or a fresh one."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    assert tuple(out.shape) == tuple(shape) and out.dtype == dtype and out.is_contiguous()
    return out


def _conv_launch(span, g, name, nbytes, device, *args, allow=()):
    """One call of a conv-family entry point sgg_<name>(desc, *args, ws, ws_bytes, stream): the shared workspace (nbytes = 0:
    NULL), the profiler span (span None: none), the call and the check.  A status in `allow` is returned instead of raised."""
    ws = workspace(nbytes, device) if nbytes else None
    pr = _prof(span, g) if span else None
    if pr: pr.start()
    rc = getattr(A.lib(), "sgg_" + name)(C.byref(g.desc), *args, _p(ws), nbytes, _s())
    if rc not in allow:
        A.check(rc, name)
    if pr: pr.stop()
    return rc


def _stats_rows(g, chunks, out_partial, device, side="y"):
    shape = g.y_shape if side == "y" else g.x_shape
    return _out(out_partial, (shape[0], chunks, shape[3], 2), torch.float32, device)


def conv_fwd(g: ConvGeom, x, w_fwd, bias, act=A.ACT_NONE, leak=0.0, out=None):
    assert tuple(x.shape) == g.x_shape and not g.is_deconv, (tuple(x.shape), g.x_shape)
    y = _out(out, g.y_shape, x.dtype, x.device)
    _conv_launch("conv2d_fwd", g, "conv2d_fwd", g.ws_fwd, x.device, _p(x), _p(w_fwd), _p(bias), _p(y), act, leak)
    return y


def conv_fwd_stats(g: ConvGeom, x, w_fwd, bias, out=None, out_partial=None):
    """conv forward (no activation) + the per-chunk (sum, sumsq) rows of its output for the instance norm that follows."""
    assert tuple(x.shape) == g.x_shape and not g.is_deconv and g.stats_chunks > 0
    y = _out(out, g.y_shape, x.dtype, x.device)
    partial = _stats_rows(g, g.stats_chunks, out_partial, x.device)
    _conv_launch("conv2d_fwd", g, "conv2d_fwd_stats", g.ws_fwd, x.device, _p(x), _p(w_fwd), _p(bias), _p(y), _p(partial))
    return y, partial


def conv_fwd_stats_pair(g: ConvGeom, x, w_fwd, bias, w_fwd2, bias2, nsplit, out=None, out_partial=None):
    """conv_fwd_stats over a stacked batch of two networks: images [:nsplit] with (w_fwd, bias), the rest with (w_fwd2, bias2)."""
    assert tuple(x.shape) == g.x_shape and g.pair_ok and g.stats_chunks > 0 and 0 < nsplit < g.x_shape[0]
    y = _out(out, g.y_shape, x.dtype, x.device)
    partial = _stats_rows(g, g.stats_chunks, out_partial, x.device)
    _conv_launch("conv2d_fwd_pair", g, "conv2d_fwd_stats_pair", g.ws_fwd, x.device,
                 _p(x), _p(w_fwd), _p(bias), _p(w_fwd2), _p(bias2), nsplit, _p(y), _p(partial))
    return y, partial


def conv_fwd_stats_normload(g: ConvGeom, x_raw, x_stats, gamma, beta, w_fwd, bias, pair=None, out=None, out_partial=None, out_norm=None):
    """conv(relu(instnorm(x_raw))) with the norm applied to the operand tiles inside the conv kernel ("normalise on load",
    sgg_conv2d_fwd_stats_normload).  x_stats: (mean, rstd) of x_raw (instnorm_finalize).  pair = (gamma2, beta2, w_fwd2,
    bias2, nsplit) for the lockstep pair.  Returns (x_norm, y, partial): the normalised operand (a by-product the backward
    pass needs), the conv output and its statistics rows -- all bit-identical to instnorm_fwd_partial + conv_fwd_stats."""
    assert tuple(x_raw.shape) == g.x_shape and g.normload_ok and g.stats_chunks > 0
    x_norm = _out(out_norm, g.x_shape, x_raw.dtype, x_raw.device)
    y = _out(out, g.y_shape, x_raw.dtype, x_raw.device)
    partial = _stats_rows(g, g.stats_chunks, out_partial, x_raw.device)
    gamma2, beta2, w2, bias2, nsplit = pair if pair is not None else (None, None, None, None, 0)
    _conv_launch("conv2d_fwd_normload" + ("_pair" if pair is not None else ""), g, "conv2d_fwd_stats_normload", g.ws_fwd, x_raw.device,
                 _p(x_raw), _p(x_stats), _p(gamma), _p(beta), _p(gamma2), _p(beta2), _p(x_norm), _p(w_fwd), _p(bias), _p(w2), _p(bias2), nsplit,
                 _p(y), _p(partial))
    return x_norm, y, partial


def instnorm_finalize(partial, HW, eps=1e-3):
    """(mean, rstd)[N][C] from a conv's statistics rows partial[N][chunks][C][2] (no pass over the tensor)."""
    N, chunks, Cp, _ = partial.shape
    stats = torch.empty((N, Cp, 2), dtype=torch.float32, device=partial.device)
    A.check(A.lib().sgg_instnorm_finalize(_p(partial), chunks, _p(stats), N, HW, Cp, eps, _s()), "instnorm_finalize")
    return stats


def conv_dgrad_pair(g: ConvGeom, dy, w_dgrad, w_dgrad2, nsplit, addend=None, out=None):
    assert tuple(dy.shape) == g.y_shape and g.pair_ok and 0 < nsplit < g.y_shape[0]
    assert addend is None or (tuple(addend.shape) == g.x_shape and addend.dtype == dy.dtype)
    dx = _out(out, g.x_shape, dy.dtype, dy.device)
    _conv_launch("conv2d_bwd_data_pair", g, "conv2d_bwd_data_pair", g.ws_dgrad, dy.device,
                 _p(dy), _p(w_dgrad), _p(w_dgrad2), nsplit, _p(addend), _p(dx))
    return dx


def conv_dgrad(g: ConvGeom, dy, w_dgrad, addend=None, out_f32=False, out=None):
    """dx = conv^T(dy) (+ addend: the skip-connection gradient, fused into the epilogue).  out_f32 (mixed mode, needs
    g.dgrad_mixed): bf16 operands, dx in float32; the addend may then be bf16 or float32."""
    assert tuple(dy.shape) == g.y_shape and not g.is_deconv
    if out_f32:
        assert g.dgrad_mixed and dy.dtype == torch.bfloat16
        assert addend is None or (tuple(addend.shape) == g.x_shape and addend.dtype in (torch.bfloat16, torch.float32))
        dx = _out(out, g.x_shape, torch.float32, dy.device)
        _conv_launch("conv2d_bwd_data", g, "conv2d_bwd_data_mixed", g.ws_dgrad, dy.device,
                     _p(dy), _p(w_dgrad), _p(addend), int(addend is not None and addend.dtype == torch.float32), _p(dx))
        return dx
    assert addend is None or (tuple(addend.shape) == g.x_shape and addend.dtype == dy.dtype)
    dx = _out(out, g.x_shape, dy.dtype, dy.device)
    _conv_launch("conv2d_bwd_data", g, "conv2d_bwd_data", g.ws_dgrad, dy.device, _p(dy), _p(w_dgrad), _p(addend), _p(dx))
    return dx


def conv_dgrad_stats(g: ConvGeom, dy, w_dgrad, addend, norm_x, norm_stats, norm_gamma, norm_beta, norm_act=A.ACT_NONE, norm_leak=0.0,
                     out=None, out_partial=None):
    """conv_dgrad + the first pass of the instance-norm backward that consumes dx (the norm whose input is norm_x)."""
    assert tuple(dy.shape) == g.y_shape and not g.is_deconv and g.bwd_stats_chunks > 0
    assert tuple(norm_x.shape) == g.x_shape and norm_x.dtype == dy.dtype
    assert addend is None or (tuple(addend.shape) == g.x_shape and addend.dtype == dy.dtype)
    dx = _out(out, g.x_shape, dy.dtype, dy.device)
    partial = _stats_rows(g, g.bwd_stats_chunks, out_partial, dy.device, side="x")
    _conv_launch("conv2d_bwd_data", g, "conv2d_bwd_data_stats", g.ws_dgrad, dy.device, _p(dy), _p(w_dgrad), _p(addend), _p(dx),
                 _p(norm_x), _p(norm_stats), _p(norm_gamma), _p(norm_beta), norm_act, norm_leak, _p(partial))
    return dx, partial


def conv_wgrad(g: ConvGeom, x, dy, dw, accumulate=False):
    """dw: f32 (R,S,C_real,K_real) view to write / accumulate into."""
    assert tuple(x.shape) == g.x_shape and tuple(dy.shape) == g.y_shape and dw.dtype == torch.float32
    _conv_launch("conv2d_bwd_weight", g, "conv2d_bwd_weight", g.ws_wgrad, x.device, _p(x), _p(dy), _p(dw), dw.shape[2], dw.shape[3], int(accumulate))


def conv_wgrad_pair(g: ConvGeom, x0, dy0, x1, dy1, dw, accumulate=False):
    """dw (+)= wgrad(x0, dy0) + wgrad(x1, dy1): two applications of one layer, one launch (needs g.wgrad_pair)."""
    assert g.wgrad_pair and dw.dtype == torch.float32
    for x, dy in ((x0, dy0), (x1, dy1)):
        assert tuple(x.shape) == g.x_shape and tuple(dy.shape) == g.y_shape
    _conv_launch("conv2d_bwd_weight_pair", g, "conv2d_bwd_weight_pair", g.ws_wgrad, x0.device,
                 _p(x0), _p(dy0), _p(x1), _p(dy1), _p(dw), dw.shape[2], dw.shape[3], int(accumulate))


def conv_wgrad_pair2(g: ConvGeom, net_a, net_b, accumulate=False):
    """Two networks of one architecture, each applied twice: net = (x0, dy0, x1, dy1, dw); ONE launch, half the slabs per network.
    Returns False (nothing launched) when the shape has no such form."""
    assert g.wgrad_pair
    dwa, dwb = net_a[4], net_b[4]
    assert dwa.dtype == torch.float32 and dwb.dtype == torch.float32 and dwa.shape == dwb.shape
    for x0, d0, x1, d1, _ in (net_a, net_b):
        for x, dy in ((x0, d0), (x1, d1)):
            assert tuple(x.shape) == g.x_shape and tuple(dy.shape) == g.y_shape
    rc = _conv_launch("conv2d_bwd_weight_pair2", g, "conv2d_bwd_weight_pair2", g.ws_wgrad, dwa.device,
                      *[_p(t) for t in net_a], *[_p(t) for t in net_b], dwa.shape[2], dwa.shape[3], int(accumulate), allow=(A.EUNSUPPORTED,))
    return rc != A.EUNSUPPORTED


# ---- grouped launches (sgg_*_group2): the same call site of two networks in one call.  `g` is ONE network's geometry; the tensors
# hold 2N images, the first network's first.  Bit-identical to two single calls.
def _stacked(shape):
    return (2 * shape[0],) + tuple(shape[1:])


def conv_fwd_group2(g: ConvGeom, x, w_fwd, bias, w_fwd2, bias2, act=A.ACT_NONE, leak=0.0, out=None):
    assert tuple(x.shape) == _stacked(g.x_shape) and not g.is_deconv
    y = _out(out, _stacked(g.y_shape), x.dtype, x.device)
    _conv_launch("conv2d_fwd_group2", g, "conv2d_fwd_group2", 2 * g.ws_fwd, x.device,
                 _p(x), _p(w_fwd), _p(bias), _p(w_fwd2), _p(bias2), _p(y), act, leak)
    return y


def conv_dgrad_group2(g: ConvGeom, dy, w_dgrad, w_dgrad2, addend=None, out=None):
    assert tuple(dy.shape) == _stacked(g.y_shape) and not g.is_deconv
    assert addend is None or (tuple(addend.shape) == _stacked(g.x_shape) and addend.dtype == dy.dtype)
    dx = _out(out, _stacked(g.x_shape), dy.dtype, dy.device)
    _conv_launch("conv2d_bwd_data_group2", g, "conv2d_bwd_data_group2", 2 * g.ws_dgrad, dy.device,
                 _p(dy), _p(w_dgrad), _p(w_dgrad2), _p(addend), _p(dx))
    return dx


def conv_wgrad_group2(g: ConvGeom, x, dy, dw, dw2, accumulate=False):
    """dw (+)= wgrad(x[:N], dy[:N]), dw2 (+)= wgrad(x[N:], dy[N:]): both networks' slabs, one reduce launch."""
    assert tuple(x.shape) == _stacked(g.x_shape) and tuple(dy.shape) == _stacked(g.y_shape) and dw.shape == dw2.shape
    _conv_launch("bwd_weight_group2", g, ("deconv2d" if g.is_deconv else "conv2d") + "_bwd_weight_group2", 2 * g.ws_wgrad, x.device,
                 _p(x), _p(dy), _p(dw), _p(dw2), dw.shape[2], dw.shape[3], int(accumulate))


def deconv_fwd_group2(g: ConvGeom, x, w_dgrad, bias, w_dgrad2, bias2, act=A.ACT_NONE, leak=0.0, out=None):
    assert tuple(x.shape) == _stacked(g.x_shape) and g.is_deconv
    y = _out(out, _stacked(g.y_shape), x.dtype, x.device)
    _conv_launch("deconv2d_fwd_group2", g, "deconv2d_fwd_group2", 2 * g.ws_fwd, x.device,
                 _p(x), _p(w_dgrad), _p(bias), _p(w_dgrad2), _p(bias2), _p(y), act, leak)
    return y


def deconv_dgrad_group2(g: ConvGeom, dy, w_fwd, w_fwd2, out=None):
    assert tuple(dy.shape) == _stacked(g.y_shape) and g.is_deconv
    dx = _out(out, _stacked(g.x_shape), dy.dtype, dy.device)
    _conv_launch("deconv2d_bwd_data_group2", g, "deconv2d_bwd_data_group2", 2 * g.ws_dgrad, dy.device, _p(dy), _p(w_fwd), _p(w_fwd2), _p(dx))
    return dx


def deconv_fwd(g: ConvGeom, x, w_dgrad, bias, act=A.ACT_NONE, leak=0.0, out=None):
    assert tuple(x.shape) == g.x_shape and g.is_deconv
    y = _out(out, g.y_shape, x.dtype, x.device)
    _conv_launch(None, g, "deconv2d_fwd", g.ws_fwd, x.device, _p(x), _p(w_dgrad), _p(bias), _p(y), act, leak)
    return y


def deconv_fwd_stats(g: ConvGeom, x, w_dgrad, bias, pair=None, out=None, out_partial=None):
    """Conv2DTranspose forward (no activation) + the per-chunk (sum, sumsq) rows of its output for the instance norm behind it.
    pair = (w_dgrad2, bias2, nsplit): `g` describes a stacked batch of two networks, images >= nsplit use the second weight set."""
    assert tuple(x.shape) == g.x_shape and g.is_deconv and g.stats_chunks > 0
    y = _out(out, g.y_shape, x.dtype, x.device)
    partial = _stats_rows(g, g.stats_chunks, out_partial, x.device)
    w2, b2, ns = pair if pair is not None else (None, None, 0)
    _conv_launch("deconv2d_fwd_stats", g, "deconv2d_fwd_stats", 0, x.device, _p(x), _p(w_dgrad), _p(bias), _p(w2), _p(b2), int(ns), _p(y), _p(partial))
    return y, partial


def deconv_dgrad(g: ConvGeom, dy, w_fwd, out=None):
    assert tuple(dy.shape) == g.y_shape and g.is_deconv
    dx = _out(out, g.x_shape, dy.dtype, dy.device)
    _conv_launch(None, g, "deconv2d_bwd_data", g.ws_dgrad, dy.device, _p(dy), _p(w_fwd), _p(dx))
    return dx


def deconv_wgrad(g: ConvGeom, x, dy, dw, accumulate=False):
    """dw: f32 (R,S,Cout_real,Cin_real) -- the Keras transpose-kernel layout."""
    assert tuple(x.shape) == g.x_shape and tuple(dy.shape) == g.y_shape
    _conv_launch(None, g, "deconv2d_bwd_weight", g.ws_wgrad, x.device, _p(x), _p(dy), _p(dw), dw.shape[2], dw.shape[3], int(accumulate))


def bias_grad(dy, db, accumulate=False):
    """db[c] (+)= sum over all pixels of dy[..., c] for c < db.numel()."""
    Cp = dy.shape[-1]
    P = dy.numel() // Cp
    need = int(A.lib().sgg_bias_grad_workspace(P, Cp))
    ws = workspace(need, dy.device)
    A.check(A.lib().sgg_bias_grad(_p(dy), _p(db), P, Cp, db.numel(), int(accumulate), dt(dy), _p(ws), ws.numel(), _s()), "bias_grad")


def bias_grad_group2(dy, db, db2, accumulate=False):
    """Two networks' tensors stacked on the batch dimension: db (+)= colsum(dy[:N]), db2 (+)= colsum(dy[N:])."""
    Cp = dy.shape[-1]
    P = dy.numel() // Cp // 2
    need = 2 * int(A.lib().sgg_bias_grad_workspace(P, Cp))
    ws = workspace(need, dy.device)
    pr = _prof("bias_grad_group2", (P, Cp))
    if pr: pr.start()
    A.check(A.lib().sgg_bias_grad_group2(_p(dy), _p(db), _p(db2), P, Cp, db.numel(), int(accumulate), dt(dy), _p(ws), ws.numel(), _s()), "bias_grad_group2")
    if pr: pr.stop()


# ----------------------------------------------------------------------------- instance norm / activations
# instnorm_forward / instnorm_backward check, allocate, size the workspace, open the profiler span and assemble the argument list
# of the sgg_instnorm_* symbol their arguments select; the layer units of module.py call them, and the named instnorm_* functions
# below are thin calls into them.
#   addend   the tensor added to the output: the residual (after the activation; may be None), or with skip=True the skip
#            (before the activation: y = act(gamma*xhat + beta + skip), generator_unet d3 / d7)
#   partial  the (sum, sumsq) / (sum g, sum g*xhat) rows of the producing conv: the norm skips its statistics pass
#   pair     two networks of the same shape on one stacked batch (images 0..nsplit-1: first network; the rest: second):
#            (gamma2, beta2, nsplit) forward, (gamma2, beta2, nsplit, dgamma2, dbeta2) backward
# The profiler span follows from the same arguments.  Forward: the named function's name (the skip forms': without "_partial") and
# the key (shape, has residual), the skip forms' (shape, has partial); backward: the skip forms only, keyed by the shape.
def instnorm_forward(x, gamma, beta, addend, eps, act, leak, skip=False, partial=None, pair=None):
    N, H, W, Cp = x.shape
    assert gamma.numel() == Cp and beta.numel() == Cp, "gamma/beta must be channel-padded"
    if skip:
        assert tuple(addend.shape) == tuple(x.shape) and addend.dtype == x.dtype
    if partial is not None:
        assert partial.shape[0] == N and partial.shape[2] == Cp
    if pair is not None:
        assert pair[0].numel() == Cp and 0 < pair[2] < N
    name = "instnorm_fwd" + ("_skip" if skip else "") + ("_partial" if partial is not None else "") + ("_pair" if pair is not None else "")
    y = torch.empty_like(x)
    stats = torch.empty((N, Cp, 2), dtype=torch.float32, device=x.device)
    args = [_p(x), _p(gamma), _p(beta)]
    if pair is not None:
        args += [_p(pair[0]), _p(pair[1]), pair[2]]
    args += [_p(addend), _p(y), _p(stats)]
    if partial is not None:
        args += [_p(partial), partial.shape[1]]
    args += [N, H * W, Cp, eps, act, leak, dt(x)]
    if partial is None:
        ws = workspace(int(A.lib().sgg_instnorm_workspace(N, H * W, Cp)), x.device)
        args += [_p(ws), ws.numel()]
    span = "instnorm_fwd" + ("_skip" if skip else "_partial" if partial is not None else "") + ("_pair" if pair is not None else "")
    pr = _prof(span, (tuple(x.shape), (partial if skip else addend) is not None))
    if pr: pr.start()
    A.check(getattr(A.lib(), "sgg_" + name)(*args, _s()), name)
    if pr: pr.stop()
    return y, stats


def instnorm_backward(dy, x, gamma, beta, stats, dgamma, dbeta, accumulate, act, leak, y=None, partial=None, pair=None):
    """y: the stored output of the skip form, whose backward returns (dx, dskip), dskip = dy * act'(y); otherwise dx alone."""
    N, H, W, Cp = x.shape
    skip = y is not None
    mixed = dy.dtype == torch.float32 and x.dtype == torch.bfloat16        # mixed mode: f32 gradient chain, bf16 tensors
    if skip:
        assert dy.dtype == x.dtype and y.dtype == x.dtype and tuple(dy.shape) == tuple(x.shape) == tuple(y.shape)
    if partial is not None:
        assert partial.shape[0] == N and partial.shape[2] == Cp
    if pair is not None:
        assert dy.dtype == x.dtype and dgamma.numel() == pair[3].numel() and 0 < pair[2] < N
    assert not (mixed and partial is not None), "mixed mode has no partial form"
    name = "instnorm_bwd" + ("_skip" if skip else "") + ("_partial" if partial is not None else "") + ("_pair" if pair is not None else "") + \
        ("_mixed" if mixed else "")
    dx = torch.empty_like(x)
    dskip = torch.empty_like(x) if skip else None
    need = N * Cp * 16 if partial is not None else int(A.lib().sgg_instnorm_workspace(N, H * W, Cp))
    ws = workspace(need, x.device)
    args = [_p(dy)] + ([_p(y)] if skip else []) + [_p(x), _p(gamma), _p(beta)]
    if pair is not None:
        args += [_p(pair[0]), _p(pair[1]), pair[2]]
    args += [_p(stats), _p(dx)] + ([_p(dskip)] if skip else []) + [_p(dgamma), _p(dbeta)]
    if pair is not None:
        args += [_p(pair[3]), _p(pair[4])]
    if partial is not None:
        args += [_p(partial), partial.shape[1]]
    args += [N, H * W, Cp, dgamma.numel(), int(accumulate), act, leak] + ([] if mixed else [dt(x)])
    pr = _prof(name, tuple(x.shape)) if skip else None
    if pr: pr.start()
    A.check(getattr(A.lib(), "sgg_" + name)(*args, _p(ws), ws.numel(), _s()), name)
    if pr: pr.stop()
    return (dx, dskip) if skip else dx


def instnorm_fwd(x, gamma, beta, residual=None, eps=1e-3, act=A.ACT_NONE, leak=0.0):
    return instnorm_forward(x, gamma, beta, residual, eps, act, leak)


def instnorm_fwd_partial(x, partial, gamma, beta, residual=None, eps=1e-3, act=A.ACT_NONE, leak=0.0):
    """instance norm whose statistics pass was done by the producing conv (conv_fwd_stats): finalize + apply only."""
    return instnorm_forward(x, gamma, beta, residual, eps, act, leak, partial=partial)


def instnorm_bwd(dy, x, gamma, beta, stats, dgamma, dbeta, accumulate=False, act=A.ACT_NONE, leak=0.0):
    """sgg_instnorm_bwd, or sgg_instnorm_bwd_mixed when dy is f32 and x is bf16."""
    return instnorm_backward(dy, x, gamma, beta, stats, dgamma, dbeta, accumulate, act, leak)


def instnorm_bwd_partial(dy, x, partial, gamma, beta, stats, dgamma, dbeta, accumulate=False, act=A.ACT_NONE, leak=0.0):
    """instance-norm backward whose statistics pass was done by the conv data gradient that produced dy."""
    return instnorm_backward(dy, x, gamma, beta, stats, dgamma, dbeta, accumulate, act, leak, partial=partial)


def instnorm_fwd_skip(x, gamma, beta, skip, eps=1e-3, act=A.ACT_NONE, leak=0.0, partial=None):
    """partial: the producing conv's (sum, sumsq) rows (conv_fwd_stats / deconv_fwd_stats) -- the norm skips its statistics pass."""
    return instnorm_forward(x, gamma, beta, skip, eps, act, leak, skip=True, partial=partial)


def instnorm_bwd_skip(dy, y, x, gamma, beta, stats, dgamma, dbeta, accumulate=False, act=A.ACT_NONE, leak=0.0):
    """Backward of instnorm_fwd_skip from its stored output y: returns (dx, dskip), dskip = dy * act'(y)."""
    return instnorm_backward(dy, x, gamma, beta, stats, dgamma, dbeta, accumulate, act, leak, y=y)


def instnorm_fwd_pair(x, gamma, beta, gamma2, beta2, nsplit, residual=None, eps=1e-3, act=A.ACT_NONE, leak=0.0):
    return instnorm_forward(x, gamma, beta, residual, eps, act, leak, pair=(gamma2, beta2, nsplit))


def instnorm_fwd_partial_pair(x, partial, gamma, beta, gamma2, beta2, nsplit, residual=None, eps=1e-3, act=A.ACT_NONE, leak=0.0):
    return instnorm_forward(x, gamma, beta, residual, eps, act, leak, partial=partial, pair=(gamma2, beta2, nsplit))


def instnorm_bwd_pair(dy, x, gamma, beta, gamma2, beta2, nsplit, stats, dgamma, dbeta, dgamma2, dbeta2, accumulate=False,
                      act=A.ACT_NONE, leak=0.0):
    return instnorm_backward(dy, x, gamma, beta, stats, dgamma, dbeta, accumulate, act, leak, pair=(gamma2, beta2, nsplit, dgamma2, dbeta2))


def instnorm_fwd_skip_pair(x, gamma, beta, gamma2, beta2, nsplit, skip, eps=1e-3, act=A.ACT_NONE, leak=0.0, partial=None):
    """instnorm_fwd_skip of two networks on one stacked batch: y = act(IN(x) + skip) with the affine set picked by image index."""
    return instnorm_forward(x, gamma, beta, skip, eps, act, leak, skip=True, partial=partial, pair=(gamma2, beta2, nsplit))


def instnorm_bwd_skip_pair(dy, y, x, gamma, beta, gamma2, beta2, nsplit, stats, dgamma, dbeta, dgamma2, dbeta2, accumulate=False,
                           act=A.ACT_NONE, leak=0.0):
    """Backward of instnorm_fwd_skip_pair from its stored output y: (dx, dskip), both stacked like x."""
    return instnorm_backward(dy, x, gamma, beta, stats, dgamma, dbeta, accumulate, act, leak, y=y, pair=(gamma2, beta2, nsplit, dgamma2, dbeta2))


def act_fwd(x, act, leak=0.0):
    y = torch.empty_like(x)
    A.check(A.lib().sgg_act_fwd(_p(x), _p(y), x.numel(), act, leak, dt(x), _s()), "act_fwd")
    return y


def act_bwd(dy, y, act, leak=0.0):
    dx = torch.empty_like(dy)
    A.check(A.lib().sgg_act_bwd(_p(dy), _p(y), _p(dx), dy.numel(), act, leak, dt(dy), _s()), "act_bwd")
    return dx


def add(a, b):
    o = torch.empty_like(a)
    A.check(A.lib().sgg_add(_p(a), _p(b), _p(o), a.numel(), dt(a), _s()), "add")
    return o


# ----------------------------------------------------------------------------- mask / losses / optimizer
def mask_reduce_fwd(h4, mask, C_real):
    N, hh, hw, Cp = h4.shape
    _, mh, mw, Cm = mask.shape
    assert Cm == C_real and mask.dtype == torch.float32
    out = torch.empty((N, mh, mw, 1), dtype=torch.float32, device=h4.device)
    A.check(A.lib().sgg_mask_reduce_fwd(_p(h4), _p(mask), _p(out), N, hh, hw, mh, mw, C_real, Cp, dt(h4), _s()), "mask_reduce_fwd")
    return out


def mask_reduce_bwd(dout, mask, h4_shape, dtype, C_real):
    N, hh, hw, Cp = h4_shape
    _, mh, mw, _ = mask.shape
    dh4 = torch.empty(h4_shape, dtype=dtype, device=dout.device)
    A.check(A.lib().sgg_mask_reduce_bwd(_p(dout), _p(mask), _p(dh4), N, hh, hw, mh, mw, C_real, Cp, dt(dtype), _s()), "mask_reduce_bwd")
    return dh4


def bce_logits(logits, label, loss, dlogits=None, weight=1.0, gscale=1.0, accumulate_loss=False, accumulate_grad=False):
    """loss: 1-element f32 tensor written/accumulated on device (no host sync)."""
    assert logits.dtype == torch.float32
    A.check(A.lib().sgg_bce_logits(_p(logits), logits.numel(), float(label), float(weight), float(gscale), _p(loss), _p(dlogits),
                                   int(bool(accumulate_loss)) | (int(bool(accumulate_grad)) << 1), _s()), "bce_logits")


def l1_loss(a, b, C_real, loss, db=None, weight=1.0, gscale=1.0, accumulate=False, accumulate_grad=False):
    Cp = a.shape[-1]
    P = a.numel() // Cp
    ws = workspace(int(A.lib().sgg_l1_loss_workspace(P, Cp)), a.device)
    A.check(A.lib().sgg_l1_loss(_p(a), _p(b), P, C_real, Cp, float(weight), float(gscale), _p(loss), _p(db),
                                int(bool(accumulate)) | (int(bool(accumulate_grad)) << 1), dt(a), _p(ws), ws.numel(), _s()), "l1_loss")


def mse_const(x, target, loss, dx=None, weight=1.0, gscale=1.0, accumulate_loss=False, accumulate_grad=False):
    """mae_criterion(x, target*ones) (module.py:340-341): mean squared error against a constant."""
    assert x.dtype == torch.float32
    A.check(A.lib().sgg_mse_const(_p(x), x.numel(), float(target), float(weight), float(gscale), _p(loss), _p(dx),
                                  int(bool(accumulate_loss)) | (int(bool(accumulate_grad)) << 1), _s()), "mse_const")


def seg_edge_weight(seg, C_real):
    """model.py:108-119 weighted_seg: (N,H,W,Cp) colour segmentation -> f32 (N,H,W) edge indicator."""
    N, H, W, Cp = seg.shape
    out = torch.empty((N, H, W), dtype=torch.float32, device=seg.device)
    A.check(A.lib().sgg_seg_edge_weight(_p(seg), _p(out), N, H, W, C_real, Cp, dt(seg), _s()), "seg_edge_weight")
    return out


def gradloss(x, target, weight, C_real, loss, dx=None, lam=1.0, gscale=1.0, accumulate_loss=False, accumulate_grad=False):
    """gradloss_criterion (module.py:347-351) scaled by lam; optional gradient w.r.t. x."""
    N, H, W, Cp = x.shape
    need = int(A.lib().sgg_gradloss_workspace(N, H, W, C_real))
    ws = workspace(need, x.device)
    A.check(A.lib().sgg_gradloss(_p(x), _p(target), _p(weight), N, H, W, C_real, Cp, float(lam), float(gscale), _p(loss), _p(dx),
                                 int(bool(accumulate_loss)) | (int(bool(accumulate_grad)) << 1), dt(x), _p(ws), ws.numel(), _s()), "gradloss")


def ssim_loss(target, x, C_real, loss, dx=None, weight=1.0, gscale=1.0, data_range=1.0, accumulate_loss=False, accumulate_grad=False):
    """sgg_ssim_loss (csrc/ssimloss.hip): loss (+)= weight * (1 - mean SSIM(target, x)) over the 11 x 11 Gaussian
    windows inside the image; optional gradient w.r.t. x.  target, x, dx internal (N,H,W,8); loss a 1-element f32 tensor."""
    N, H, W, Cp = x.shape
    assert target.shape == x.shape and target.dtype == x.dtype and (dx is None or (dx.shape == x.shape and dx.dtype == x.dtype))
    need = int(A.lib().sgg_ssim_loss_workspace(N, H, W, int(C_real)))
    if not need:
        A.check(A.EUNSUPPORTED, f"ssim_loss {N}x{H}x{W}x{C_real}")
    ws = workspace(need, x.device)
    A.check(A.lib().sgg_ssim_loss(_p(target), _p(x), N, H, W, int(C_real), Cp, float(data_range), float(weight), float(gscale), _p(loss),
                                  _p(dx), int(bool(accumulate_loss)) | (int(bool(accumulate_grad)) << 1), dt(x), _p(ws), ws.numel(), _s()),
            "ssim_loss")


def adam(theta, g, m, v, t, lr=1e-3, beta1=0.5, beta2=0.999, eps=1e-7, grad_scale=1.0):
    assert theta.dtype == torch.float32 and theta.numel() == g.numel() == m.numel() == v.numel()
    A.check(A.lib().sgg_adam(_p(theta), _p(g), _p(m), _p(v), theta.numel(), int(t), lr, beta1, beta2, eps, grad_scale, _s()), "adam")


def _adam_args(theta, g, m, v, state, sched=None, guard=None):
    """What the entry points with a device-side counter ask of their tensors (csrc/adam.hip): f32 buffers of one length,
    ``state`` int64[2], ``sched`` int64[3] and ``guard`` float64[4] where given."""
    assert theta.dtype == torch.float32 and theta.numel() == g.numel() == m.numel() == v.numel()
    assert state.dtype == torch.int64 and state.numel() == 2
    assert sched is None or (sched.dtype == torch.int64 and sched.numel() == 3)
    assert guard is None or (guard.dtype == torch.float64 and guard.numel() == 4)


def adam_iter(theta, g, m, v, state, lr=1e-3, beta1=0.5, beta2=0.999, eps=1e-7, grad_scale=1.0):
    """Adam with the step number kept on the device (``state``: int64[2] = [iterations, scratch]; iterations is incremented)."""
    _adam_args(theta, g, m, v, state)
    A.check(A.lib().sgg_adam_iter(_p(theta), _p(g), _p(m), _p(v), theta.numel(), _p(state), lr, beta1, beta2, eps, grad_scale, _s()), "adam_iter")


def adam_sched(theta, g, m, v, state, sched, lr=1e-3, beta1=0.5, beta2=0.999, eps=1e-7, grad_scale=1.0):
    """``adam_iter`` with the base rate ``lr`` put through the linear decay of model.py:223 on the device: ``sched`` is a device
    int64[3] = [steps_per_epoch, epoch_step, epochs], read when the launch runs (``scheduled_lr`` states the rule)."""
    assert sched is not None
    _adam_args(theta, g, m, v, state, sched)
    A.check(A.lib().sgg_adam_sched(_p(theta), _p(g), _p(m), _p(v), theta.numel(), _p(state), _p(sched), lr, beta1, beta2, eps, grad_scale, _s()),
            "adam_sched")


def scheduled_lr(lr, iterations, steps_per_epoch, epoch_step, epochs):
    """The rate ``adam_sched`` applies at step number ``iterations`` (0-based: the counter before the update), as np.float32 --
    the kernel's rule in the kernel's order of evaluation, on the host (logging, tests):
    ``lr if epoch < epoch_step else lr*(epochs-epoch)/(epochs-epoch_step)`` (model.py:223) with epoch = iterations //
    steps_per_epoch, clamped at 0 past the last epoch.  ``lr`` enters as the f32 the kernel receives; the decayed rate is
    evaluated in double and rounded to f32 once."""
    lr = np.float32(lr)
    iterations, epoch_step, epochs = int(iterations), int(epoch_step), int(epochs)
    e = iterations // max(int(steps_per_epoch), 1)
    if epochs <= epoch_step or e < epoch_step:
        return lr
    return np.float32((float(lr) * float(max(epochs - e, 0))) / float(epochs - epoch_step))


GRAD_GUARD_CHUNK = 8192          # elements per block of the sum-of-squares pass (GSQ_CHUNK, csrc/adam.hip)


def grad_guard_workspace(n: int, device) -> torch.Tensor:
    """A workspace of its own for the guarded update of an ``n``-element buffer (``sgg_grad_guard_workspace`` bytes): the
    decision header is read by the update launch, so it is not taken from the shared scratch buffer."""
    return torch.zeros(int(A.lib().sgg_grad_guard_workspace(int(n))), dtype=torch.uint8, device=device)


def grad_sumsq(g, ws=None):
    """The partial pass alone (``sgg_grad_sumsq``): returns (float64 sums of squares, int32 non-finite flags), one entry per
    ``GRAD_GUARD_CHUNK`` elements of ``g`` -- views into ``ws``."""
    assert g.dtype == torch.float32
    n = g.numel()
    ws = grad_guard_workspace(n, g.device) if ws is None else ws
    A.check(A.lib().sgg_grad_sumsq(_p(g), n, _p(ws), ws.numel(), _s()), "grad_sumsq")
    chunks = (n + GRAD_GUARD_CHUNK - 1) // GRAD_GUARD_CHUNK
    rec = ws[16:16 + 16 * chunks]
    return rec.view(torch.float64)[0::2], rec.view(torch.int32)[2::4]


def adam_guard(theta, g, m, v, state, guard, ws, sched=None, lr=1e-3, beta1=0.5, beta2=0.999, eps=1e-7, grad_scale=1.0, max_norm=0.0):
    """``adam_iter`` (``sched`` None) or ``adam_sched`` behind the device-side guard (``guarded_update`` states the rule):
    ``guard`` is a device float64[4] = [last_norm, last_clip, skipped_total, applied_total], ``ws`` a ``grad_guard_workspace``."""
    assert guard is not None
    _adam_args(theta, g, m, v, state, sched, guard)
    A.check(A.lib().sgg_adam_guard(_p(theta), _p(g), _p(m), _p(v), theta.numel(), _p(state), _p(sched), lr, beta1, beta2, eps,
                                   grad_scale, float(max_norm), _p(guard), _p(ws), ws.numel(), _s()), "adam_guard")


def guarded_update(theta, g, m, v, iterations, lr=1e-3, beta1=0.5, beta2=0.999, eps=1e-7, grad_scale=1.0, max_norm=0.0, sched=None):
    """The whole rule of ``adam_guard`` in float64 NumPy (logging, tests), for one step:

        norm = sqrt(sum g^2) * grad_scale;   skip = any g is NaN or +-Inf
        clip = 1 if skip or max_norm <= 0 or norm <= max_norm else float32(max_norm / norm)
        skipped: theta, m, v and iterations stay;   otherwise Keras Adam at t = iterations + 1 on g * float32(grad_scale * clip)
        at the rate ``scheduled_lr(lr, iterations, *sched)`` (``sched`` None: ``lr``)

    ``lr``, ``grad_scale``, ``max_norm`` and the betas enter as the f32 values the kernel receives; everything else is
    float64.  Returns (theta, m, v, iterations, info) with info = {"norm", "clip", "skip"}."""
    f = np.float32
    theta, g, m, v = (np.asarray(x, dtype=np.float64) for x in (theta, g, m, v))
    gs, mx = f(grad_scale), f(max_norm)
    skip = not bool(np.isfinite(g).all())
    with np.errstate(over="ignore", invalid="ignore"):
        norm = float(np.sqrt(np.sum(g * g))) * float(gs)
    clip = f(1.0)
    if not skip and mx > 0 and not norm <= float(mx):
        clip = f(float(mx) / norm)
    info = {"norm": norm, "clip": float(clip), "skip": skip}
    if skip:
        return theta, m, v, int(iterations), info
    t = int(iterations) + 1
    b1, b2, eps = float(f(beta1)), float(f(beta2)), float(f(eps))
    lr_e = float(f(lr)) if sched is None else float(scheduled_lr(lr, iterations, *sched))
    lr_t = lr_e * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    gi = g * float(f(gs * clip))
    m = b1 * m + (1.0 - b1) * gi
    v = b2 * v + (1.0 - b2) * gi * gi
    return theta - lr_t * m / (np.sqrt(v) + eps), m, v, t, info


EMA_CHUNK = 2048                 # elements per block of the fused update and of swap_ (EMA_CHUNK, csrc/adam.hip)


def adam_ema(theta, g, m, v, ema, state, ema_state, ema_decay, sched=None, lr=1e-3, beta1=0.5, beta2=0.999, eps=1e-7, grad_scale=1.0,
             guard=None, ws=None, max_norm=0.0):
    """``adam_iter`` / ``adam_sched`` (``guard`` None) or ``adam_guard`` (``guard`` and ``ws`` given) that also keeps ``ema``, the
    exponential moving average of ``theta``, in the same launches: ``ema = d_t ema + (1 - d_t) theta_new`` with ``d_t = min(ema_decay, (1 + t) / (10 + t))``, t = iterations
    after the update (include/sggan.h).  ``ema_state`` is a device
    float32[2] = [d_t, 1 - d_t], written by the prep launch; theta, m, v, iterations and the guard record come out with the
    bits of the calls named above."""
    _adam_args(theta, g, m, v, state, sched, guard)
    assert guard is None or ws is not None
    assert ema.dtype == torch.float32 and ema.numel() == theta.numel() and ema_state.dtype == torch.float32 and ema_state.numel() == 2
    A.check(A.lib().sgg_adam_ema(_p(theta), _p(g), _p(m), _p(v), _p(ema), theta.numel(), _p(state), _p(sched), lr, beta1, beta2, eps,
                                 grad_scale, float(ema_decay), _p(ema_state), float(max_norm), int(guard is not None), _p(guard),
                                 _p(ws) if guard is not None else None, ws.numel() if guard is not None else 0, _s()), "adam_ema")


def swap_(a, b):
    """Exchange the contents of two float32 buffers of equal length bit for bit, in place, in one pass (``sgg_swap_f32``)."""
    assert a.dtype == b.dtype == torch.float32 and a.numel() == b.numel()
    A.check(A.lib().sgg_swap_f32(_p(a), _p(b), a.numel(), _s()), "swap_")


# ----------------------------------------------------------------------------- spectral norm
class SpectralTable:
    """The device item table of ``sgg_spectral_sigma`` / ``sgg_spectral_grad`` for a list of layers, with the workspaces of both
    calls.  entries: [(w, g, u, v, sigma, inv_sigma)] -- ``w`` (and ``g``, or None) the layer's f32 kernel (gradient) viewed as
    (rows, K), contiguous; ``u`` (K,), ``v`` (rows,), ``sigma`` and ``inv_sigma`` one-element f32 views.  Everything is device
    memory the caller keeps alive; the table holds the addresses, so the launches are the same every step (capturable)."""

    def __init__(self, entries, device):
        items = (A.SpectralItem * len(entries))()
        self.max_rows = self.max_K = 0
        for it, (w, g, u, v, sigma, inv_sigma) in zip(items, entries):
            rows, Kc = w.shape
            for t in (w, g, u, v, sigma, inv_sigma):
                assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32)
            assert g is None or tuple(g.shape) == (rows, Kc)
            assert u.numel() == Kc and v.numel() == rows and sigma.numel() == 1 and inv_sigma.numel() == 1
            if Kc > A.SPECTRAL_MAX_K:
                raise A.SggError(f"spectral norm: {Kc} output channels, the kernels take at most {A.SPECTRAL_MAX_K}")
            it.w, it.g, it.u, it.v = w.data_ptr(), (g.data_ptr() if g is not None else None), u.data_ptr(), v.data_ptr()
            it.sigma, it.inv_sigma, it.rows, it.K = sigma.data_ptr(), inv_sigma.data_ptr(), rows, Kc
            self.max_rows, self.max_K = max(self.max_rows, rows), max(self.max_K, Kc)
        self.n = len(entries)
        self.has_grad = all(e[1] is not None for e in entries)
        self.table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(device)
        L = A.lib()
        self.ws_sigma = torch.empty(int(L.sgg_spectral_sigma_workspace(self.n, self.max_rows, self.max_K)), dtype=torch.uint8, device=device)
        self.ws_grad = torch.empty(int(L.sgg_spectral_grad_workspace(self.n, self.max_rows)), dtype=torch.uint8, device=device)
        self.keep = entries


def spectral_sigma(tab: SpectralTable, advance=True):
    """One power iteration per item (``sgg_spectral_sigma``): v, sigma and 1 / sigma are written, u is replaced when ``advance``."""
    A.check(A.lib().sgg_spectral_sigma(_p(tab.table), tab.n, tab.max_rows, tab.max_K, 1 if advance else 0, _p(tab.ws_sigma),
                                       tab.ws_sigma.numel(), _s()), "spectral_sigma")


def spectral_grad(tab: SpectralTable):
    """dWbar -> dW in place on every item's gradient slice (``sgg_spectral_grad``)."""
    assert tab.has_grad
    A.check(A.lib().sgg_spectral_grad(_p(tab.table), tab.n, tab.max_rows, tab.max_K, _p(tab.ws_grad), tab.ws_grad.numel(), _s()),
            "spectral_grad")


# ----------------------------------------------------------------------------- data side
def seg_class_map(rgb_u8):
    """uint8 (..., M, N, 3|4) -> uint8 (..., M, N) class indices (segment_class.py:60-99), bit exact."""
    assert rgb_u8.dtype == torch.uint8 and rgb_u8.shape[-1] >= 3
    out = torch.empty(rgb_u8.shape[:-1], dtype=torch.uint8, device=rgb_u8.device)
    A.check(A.lib().sgg_seg_class_map(_p(rgb_u8), rgb_u8.shape[-1], out.numel(), _p(out), _s()), "seg_class_map")
    return out


def onehot_resample(idx_u8, oh, ow, n_classes):
    N, H, W = idx_u8.shape
    mask = torch.empty((N, oh, ow, n_classes), dtype=torch.float32, device=idx_u8.device)
    A.check(A.lib().sgg_onehot_resample(_p(idx_u8), _p(mask), N, H, W, oh, ow, n_classes, _s()), "onehot_resample")
    return mask


def resample_u8(src_u8, index, flip, rows, cols, out, C):
    """Band-table resample of device-resident uint8 sources straight into a batch in the internal layout (sgg_resample_u8).
    src_u8 (M,H0,W0,3|4) uint8; index / flip int32 (N,) device tensors; rows / cols: (weights f32 (n_out,taps), starts int32
    (n_out,), step) device band tables (data.band_table); out (N,H,W,cpad(C)) bf16 / f32, written in full."""
    M, H0, W0, Cs = src_u8.shape
    N, H, W, Cp = out.shape
    (rw, rs, _), (cw, cs, cstep) = rows, cols
    assert src_u8.dtype == torch.uint8 and index.dtype == flip.dtype == rs.dtype == cs.dtype == torch.int32
    assert rw.dtype == cw.dtype == torch.float32 and Cp == A.CPAD and index.numel() == flip.numel() == N
    assert tuple(rw.shape) == (H, rw.shape[1]) and tuple(cw.shape) == (W, cw.shape[1]) and rs.numel() == H and cs.numel() == W
    A.check(A.lib().sgg_resample_u8(_p(src_u8), M, H0, W0, Cs, _p(index), _p(flip), _p(rw), _p(rs), rw.shape[1],
                                    _p(cw), _p(cs), cw.shape[1], int(cstep), _p(out), N, H, W, int(C), dt(out), _s()), "resample_u8")
    return out


def warp_affine_u8(src_u8, index, matrices, cols, window, out):
    """The augmented copy's warp (sgg_warp_affine_u8): src_u8 (M,S,W0,3|4) uint8; index int32 (N,), matrices float64 (N,2,2,3)
    (data.augment_matrices), cols = device band table of the squaring stage (data.band_table((W0, S))); window = (rows, cols)
    of data.warp_window; out (N,S,S,4) f32, written in full."""
    M, S, W0, Cs = src_u8.shape
    N = out.shape[0]
    cw, cs, _ = cols
    assert src_u8.dtype == torch.uint8 and index.dtype == cs.dtype == torch.int32 and index.numel() == N
    assert matrices.dtype == torch.float64 and tuple(matrices.shape) == (N, 2, 2, 3)
    assert cw.dtype == out.dtype == torch.float32 and tuple(out.shape) == (N, S, S, 4) and tuple(cw.shape) == (S, cw.shape[1]) and cs.numel() == S
    A.check(A.lib().sgg_warp_affine_u8(_p(src_u8), M, S, W0, Cs, _p(index), _p(matrices), _p(cw), _p(cs), cw.shape[1],
                                       int(window[0]), int(window[1]), _p(out), N, _s()), "warp_affine_u8")
    return out


def resample_f32(src, flip, rows, cols, out, C):
    """resample_u8 over an f32 source (N,H0,W0,4) (sgg_resample_f32): source sample n -> out[n].  ``out`` (N,H,W,cpad) bf16 /
    f32 may be a view with a sample stride (``buf[1::2]``: the copies' rows of a doubled batch), dense within a sample."""
    N, H0, W0, c4 = src.shape
    No, H, W, Cp = out.shape
    (rw, rs, _), (cw, cs, cstep) = rows, cols
    assert src.dtype == torch.float32 and c4 == 4 and src.is_contiguous() and flip.dtype == rs.dtype == cs.dtype == torch.int32
    assert rw.dtype == cw.dtype == torch.float32 and Cp == A.CPAD and No == N and flip.numel() == N and out.is_cuda
    assert tuple(rw.shape) == (H, rw.shape[1]) and tuple(cw.shape) == (W, cw.shape[1]) and rs.numel() == H and cs.numel() == W
    assert tuple(out.stride()[1:]) == (W * Cp, Cp, 1) and (N == 1 or out.stride(0) >= H * W * Cp)
    stride = out.stride(0) if N > 1 else H * W * Cp
    out_p = _p(out[0])                      # the first sample's address: the view as a whole need not be contiguous
    A.check(A.lib().sgg_resample_f32(_p(src), N, H0, W0, _p(flip), _p(rw), _p(rs), rw.shape[1], _p(cw), _p(cs), cw.shape[1],
                                     int(cstep), out_p, stride, H, W, int(C), dt(out), _s()), "resample_f32")
    return out


def pad_channels(x_f32, Cd, dtype, out=None):
    Cs = x_f32.shape[-1]
    out = _out(out, tuple(x_f32.shape[:-1]) + (Cd,), dtype, x_f32.device)
    A.check(A.lib().sgg_pad_channels(_p(x_f32), _p(out), x_f32.numel() // Cs, Cs, Cd, dt(dtype), _s()), "pad_channels")
    return out


def unpad_channels(x, Cd):
    Cs = x.shape[-1]
    out = torch.empty(x.shape[:-1] + (Cd,), dtype=torch.float32, device=x.device)
    A.check(A.lib().sgg_unpad_channels(_p(x), _p(out), x.numel() // Cs, Cs, Cd, dt(x), _s()), "unpad_channels")
    return out


# ----------------------------------------------------------------------------- dense CRF (metric.dense_crf)
def dense_crf_workspace_bytes(H, W, C):
    """Bytes of workspace sgg_dense_crf needs for a (C,H,W) problem; 0: the shape is not supported."""
    return int(A.lib().sgg_dense_crf_workspace_bytes(int(H), int(W), int(C)))


def dense_crf(img_u8, probs=None, unary=None, max_iter=10, pos_w=3.0, pos_xy_std=1.0, bi_w=4.0, bi_xy_std=67.0, bi_rgb_std=3.0,
              out=None, workspace=None):
    """Exact mean-field dense CRF (sgg_dense_crf): img_u8 (H,W,3) uint8 and either probs (C,H,W) f32 (the unary
    -log(clip(p, 1e-5, 1)) is taken on the device) or a ready unary (C,H,W) f32 -> Q (C,H,W) f32 after max_iter steps.
    ``workspace``: a uint8 device tensor of at least dense_crf_workspace_bytes(H, W, C) bytes (allocated when None)."""
    assert (probs is None) != (unary is None), "give probs or unary, not both"
    src = probs if unary is None else unary
    C_, H, W = src.shape
    assert img_u8.dtype == torch.uint8 and tuple(img_u8.shape) == (H, W, 3) and src.dtype == torch.float32
    need = dense_crf_workspace_bytes(H, W, C_)
    if need == 0:
        A.check(A.EUNSUPPORTED, f"dense_crf {C_}x{H}x{W}")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=src.device)
    assert workspace.dtype == torch.uint8
    out = _out(out, (C_, H, W), torch.float32, src.device)
    A.check(A.lib().sgg_dense_crf(_p(img_u8), _p(probs), _p(unary), H, W, C_, int(max_iter), float(pos_w), float(pos_xy_std),
                                  float(bi_w), float(bi_xy_std), float(bi_rgb_std), _p(out), _p(workspace), workspace.numel(), _s()),
            "dense_crf")
    return out


# ----------------------------------------------------------------------------- class-level evaluation (csrc/evalseg.hip)
def _palette_args(palette):
    """(keys, classes, K) for the C ABI from ``(keys, classes)`` host arrays; None -> the library's built-in table."""
    if palette is None:
        return None, None, 0, ()
    keys = np.ascontiguousarray(palette[0], dtype=np.uint32)
    classes = np.ascontiguousarray(palette[1], dtype=np.uint8)
    assert keys.ndim == 1 and keys.shape == classes.shape, "palette: (keys uint32[K], classes uint8[K])"
    return keys.ctypes.data_as(C.c_void_p), classes.ctypes.data_as(C.c_void_p), int(keys.size), (keys, classes)


def _pixel_input(img):
    """A contiguous device image (N,H,W,Cs) -> (tensor, kind): f32 / bf16 with Cs >= 3, or uint8 with Cs = 3 | 4."""
    assert img.is_cuda and img.dim() == 4, "device image (N,H,W,C) required"
    if img.dtype == torch.uint8:
        return img.contiguous(), A.SGG_U8
    return img.contiguous(), dt(img)


def palette_decode(img, palette=None, other_class=0, max_dist2=-1, labels=None, truth=None, select=None, n_class=0, hist=None,
                   want_labels=True):
    """sgg_palette_decode: img (N,H,W,Cs) -> labels int32 (N,H,W) (``want_labels``) and / or, with ``truth`` uint8 (N,H,W) and
    ``hist`` int64 [n_class^2], the confusion counts added into ``hist`` (only where ``select`` uint8 (N,H,W) is non-zero, when
    given).  One launch.  Returns (labels or None, hist or None)."""
    img, kind = _pixel_input(img)
    N, H, W, Cs = img.shape
    if want_labels:
        labels = _out(labels, (N, H, W), torch.int32, img.device)
    for t in (truth, select):
        assert t is None or (t.dtype == torch.uint8 and tuple(t.shape) == (N, H, W))
    assert hist is None or (hist.dtype == torch.int64 and hist.numel() == n_class * n_class)
    keys, classes, K_, keep = _palette_args(palette)
    A.check(A.lib().sgg_palette_decode(_p(img), kind, N * H * W, Cs, keys, classes, K_, int(other_class), int(max_dist2),
                                       _p(labels) if want_labels else None, _p(truth), _p(select), int(n_class), _p(hist), _s()),
            "palette_decode")
    return (labels if want_labels else None), hist


def palette_probs(img, n_class, palette=None, sigma=32.0, other_class=0, max_dist2=-1, out=None):
    """sgg_palette_probs: img (N,H,W,Cs) -> class probabilities f32 (N,n_class,H,W), the ``probs`` of dense_crf."""
    img, kind = _pixel_input(img)
    N, H, W, Cs = img.shape
    out = _out(out, (N, int(n_class), H, W), torch.float32, img.device)
    keys, classes, K_, keep = _palette_args(palette)
    A.check(A.lib().sgg_palette_probs(_p(img), kind, N, H * W, Cs, keys, classes, K_, int(other_class), int(max_dist2), int(n_class),
                                      float(sigma), _p(out), _s()), "palette_probs")
    return out


def class_boundary_band(cls_u8, r, out=None):
    """sgg_class_boundary_band: class map uint8 (N,H,W) -> uint8 (N,H,W), 1 where a pixel within r (Chebyshev, inside the image)
    has another class."""
    assert cls_u8.dtype == torch.uint8 and cls_u8.dim() == 3
    N, H, W = cls_u8.shape
    out = _out(out, (N, H, W), torch.uint8, cls_u8.device)
    A.check(A.lib().sgg_class_boundary_band(_p(cls_u8), _p(out), N, H, W, int(r), _s()), "class_boundary_band")
    return out


# ----------------------------------------------------------------------------- paired image quality (csrc/imgqual.hip)
def image_quality_workspace_bytes(N, H, W):
    """Bytes of workspace sgg_image_quality needs for N pairs of H x W images; 0: the shape is not supported."""
    return int(A.lib().sgg_image_quality_workspace(int(N), int(H), int(W)))


def image_quality(a, b, out=None, workspace=None):
    """sgg_image_quality: two device images (N,H,W,Cs), each f32 / bf16 (Cs >= 3, values in [-1,1]) or uint8 (Cs = 3 | 4) ->
    (N,3) float64 device tensor {sum |a-b|, sum (a-b)^2, sum of the SSIM map} over the 8-bit colours.  Two launches, no sync.
    ``workspace``: a uint8 device tensor of at least image_quality_workspace_bytes(N, H, W) bytes (allocated when None)."""
    a, kind_a = _pixel_input(a)
    b, kind_b = _pixel_input(b)
    N, H, W, Ca = a.shape
    assert tuple(b.shape[:3]) == (N, H, W), f"image_quality: {tuple(a.shape)} against {tuple(b.shape)}"
    need = image_quality_workspace_bytes(N, H, W)
    if need == 0:
        A.check(A.EUNSUPPORTED, f"image_quality {N}x{H}x{W}")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=a.device)
    assert workspace.dtype == torch.uint8
    out = _out(out, (N, 3), torch.float64, a.device)
    A.check(A.lib().sgg_image_quality(_p(a), kind_a, Ca, _p(b), kind_b, b.shape[3], N, H, W, _p(out), _p(workspace), workspace.numel(),
                                      _s()), "image_quality")
    return out


# ----------------------------------------------------------------------------- differentiable augmentation (csrc/diffaug.hip)
DIFFAUG_COLOR, DIFFAUG_CUTOUT = 1, 2
DIFFAUG_CHUNK = 2048             # pixels per block of the partial-sum and apply passes (DA_CHUNK, csrc/diffaug.hip)


def diffaug_policy_bits(policy) -> int:
    """'color,cutout' | 'color' | 'cutout' -> policy bits; None / '' -> 0 (off)."""
    bits = 0
    for word in (policy or "").replace(" ", "").split(","):
        if word == "color":
            bits |= DIFFAUG_COLOR
        elif word == "cutout":
            bits |= DIFFAUG_CUTOUT
        elif word:
            raise ValueError(f"diffaug policy '{policy}': unknown word '{word}' (color, cutout)")
    return bits


def diffaug_draw(params, iterations, seed, sample_offset, stream_id, H, W, policy_bits, brightness=0.25):
    """sgg_diffaug_draw: fill the (rows, 8) f32 device table ``params`` with the rows of samples sample_offset .. + rows for the
    draw stream ``stream_id`` (2 * which_D + role) at the step ``iterations`` (a 1-element int64 DEVICE tensor) holds when the
    launch runs.  One launch, no host state."""
    assert params.dtype == torch.float32 and params.dim() == 2 and params.shape[1] == 8
    assert iterations.dtype == torch.int64 and iterations.is_cuda
    A.check(A.lib().sgg_diffaug_draw(_p(params), params.shape[0], C.c_void_p(iterations.data_ptr()), int(seed) & 0xffffffff,
                                     int(sample_offset), int(stream_id), int(H), int(W), int(policy_bits), float(brightness), _s()),
            "diffaug_draw")
    return params


def _diffaug_ws(rows, H, W, device):
    need = int(A.lib().sgg_diffaug_workspace(rows, H, W))
    if need == 0:
        A.check(A.EUNSUPPORTED, f"diffaug {rows}x{H}x{W}")
    return workspace(need, device)


def diffaug(x, params, C_real, out=None):
    """sgg_diffaug_fwd: x internal (rows,H,W,8) -> the augmented copy (never in place), one parameter row per image."""
    rows, H, W, Cp = x.shape
    assert params.dtype == torch.float32 and tuple(params.shape) == (rows, 8)
    out = _out(out, tuple(x.shape), x.dtype, x.device)
    ws = _diffaug_ws(rows, H, W, x.device)
    A.check(A.lib().sgg_diffaug_fwd(_p(x), _p(out), _p(params), rows, H, W, int(C_real), Cp, dt(x), _p(ws), ws.numel(), _s()), "diffaug")
    return out


def diffaug_bwd(dy, params, C_real, addend=None, out=None):
    """sgg_diffaug_bwd: the adjoint of diffaug for the gradient dy of its output (+ addend, joined once)."""
    rows, H, W, Cp = dy.shape
    assert params.dtype == torch.float32 and tuple(params.shape) == (rows, 8)
    assert addend is None or (addend.shape == dy.shape and addend.dtype == dy.dtype)
    out = _out(out, tuple(dy.shape), dy.dtype, dy.device)
    ws = _diffaug_ws(rows, H, W, dy.device)
    A.check(A.lib().sgg_diffaug_bwd(_p(dy), _p(params), _p(addend), _p(out), rows, H, W, int(C_real), Cp, dt(dy), _p(ws), ws.numel(),
                                    _s()), "diffaug_bwd")
    return out


# ----------------------------------------------------------------------------- training-mode dropout (csrc/dropout.hip)
DROPOUT_THREADS, DROPOUT_CHUNK, DROPOUT_GRID_BLOCKS = 256, 1024, 2048     # DO_THREADS, DO_CHUNK (vectors of 8), DO_GRID_BLOCKS


def dropout_threshold(rate) -> int:
    """round(rate * 65536) clamped to 0..65535: an element is dropped iff its 16-bit draw is below it, probability threshold / 65536."""
    rate = float(rate)
    if not 0.0 <= rate < 1.0:
        raise ValueError(f"dropout rate must lie in [0, 1), got {rate!r}")
    return min(max(int(round(rate * 65536.0)), 0), 65535)


def dropout_(x, rate, iterations, seed, sample_offset, stream_id):
    """sgg_dropout, in place on x (n_samples, ...): elements dropped with probability ``rate`` become +0, the others are scaled by
    1 / (1 - rate).  The mask comes from (the step ``iterations``, a 1-element int64 DEVICE tensor, holds when the launch runs;
    seed; stream_id; sample_offset + row; element index) and from nothing else: the same call on the gradient is the backward."""
    assert iterations.dtype == torch.int64 and iterations.is_cuda
    if x.numel():
        n = x.shape[0]
        A.check(A.lib().sgg_dropout(_p(x), n, x.numel() // n, dropout_threshold(rate), C.c_void_p(iterations.data_ptr()),
                                    int(seed) & 0xffffffff, int(sample_offset), int(stream_id), dt(x), _s()), "dropout")
    return x


# ----------------------------------------------------------------------------- 2x resampling of the resize-convolution layers (csrc/upsample.hip)
UPSAMPLE_THREADS, UPSAMPLE_CHUNK, UPSAMPLE_GRID_BLOCKS = 256, 256, 1024     # UP_THREADS, UP_CHUNK (low-resolution vectors of 8), UP_GRID_BLOCKS
UPSAMPLE_MODES = {"nearest": A.UPSAMPLE_NEAREST, "bilinear": A.UPSAMPLE_BILINEAR}


def upsample_mode(mode) -> int:
    try:
        return UPSAMPLE_MODES[mode]
    except (KeyError, TypeError):
        raise ValueError(f"upsample2x mode must be one of {', '.join(UPSAMPLE_MODES)}, got {mode!r}")


def upsample2x(x, mode, out=None):
    """sgg_upsample2x_fwd: x internal (N,H,W,Cp) -> (N,2H,2W,Cp), ``mode`` 'nearest' (a copy) or 'bilinear' (half-pixel centres)."""
    m = upsample_mode(mode)
    N, H, W, Cp = x.shape
    out = _out(out, (N, 2 * H, 2 * W, Cp), x.dtype, x.device)
    A.check(A.lib().sgg_upsample2x_fwd(_p(x), _p(out), N, H, W, Cp, m, dt(x), _s()), "upsample2x")
    return out


def upsample2x_bwd(dy, mode, out=None):
    """sgg_upsample2x_bwd: the adjoint of upsample2x for the gradient dy (N,2H,2W,Cp) of its output -> (N,H,W,Cp)."""
    m = upsample_mode(mode)
    N, H2, W2, Cp = dy.shape
    if H2 % 2 or W2 % 2:
        raise ValueError(f"upsample2x_bwd: dy {tuple(dy.shape)} is no output of upsample2x (odd height or width)")
    out = _out(out, (N, H2 // 2, W2 // 2, Cp), dy.dtype, dy.device)
    A.check(A.lib().sgg_upsample2x_bwd(_p(dy), _p(out), N, H2 // 2, W2 // 2, Cp, m, dt(dy), _s()), "upsample2x_bwd")
    return out


# ----------------------------------------------------------------------------- feature-matching loss (csrc/featmatch.hip)
FEATMATCH_THREADS, FEATMATCH_CHUNK = 256, 4096     # FM_THREADS, FM_CHUNK (16-byte vectors per block)


def _fm_check(reals, fakes, c_reals):
    L = len(fakes)
    if not 1 <= L <= A.FM_MAX_PAIRS or len(reals) != L or len(c_reals) != L:
        raise ValueError(f"feature_match: 1..{A.FM_MAX_PAIRS} pairs with one C_real each, got {len(reals)} reals, {L} fakes, {len(c_reals)} C_real")
    for i, (r, f, c) in enumerate(zip(reals, fakes, c_reals)):
        if tuple(r.shape) != tuple(f.shape) or r.dtype != f.dtype or f.dtype != fakes[0].dtype:
            raise ValueError(f"feature_match: pair {i}: real {tuple(r.shape)} {r.dtype} against fake {tuple(f.shape)} {f.dtype} "
                             f"(all pairs in {fakes[0].dtype})")
        if f.dim() < 2 or f.numel() == 0 or f.shape[-1] % A.CPAD or not 1 <= int(c) <= f.shape[-1]:
            raise ValueError(f"feature_match: pair {i}: {tuple(f.shape)} with C_real {c}: channels padded to a multiple of {A.CPAD}, "
                             "1 <= C_real <= Cpad, no empty tensor")
    return L


def feature_match(reals, fakes, c_reals, loss, term, weight, accumulate_loss=False, out=None):
    """sgg_feature_match: ``term`` = the mean over the L pairs of mean |fake_i - real_i| over the real channels,
    ``loss`` (+)= weight * term, both 1-element f32 device tensors; returns [grad_i] = weight / (L * count_i) * sign(fake_i - real_i)
    in the storage type (the reals are constants; ``out``: the caller's buffers for them).  Two launches for any L; the pair table
    travels in the kernel arguments."""
    L = _fm_check(reals, fakes, c_reals)
    grads = [torch.empty_like(f) for f in fakes] if out is None else list(out)
    if len(grads) != L or any(g.shape != f.shape or g.dtype != f.dtype for g, f in zip(grads, fakes)):
        raise ValueError("feature_match: out must hold one buffer per pair, shaped and typed like its fake")
    if any(s.dtype != torch.float32 or s.numel() != 1 for s in (loss, term)):
        raise ValueError("feature_match: loss and term are 1-element float32 tensors")
    for t in list(reals) + list(fakes) + grads + [loss, term]:          # (before any address is taken: the kernel walks flat memory)
        if not (t.is_cuda and t.is_contiguous()):
            raise ValueError("feature_match: device-resident contiguous tensors required")
    pairs = (A.FmPair * L)(*[A.FmPair(r.data_ptr(), f.data_ptr(), g.data_ptr(), f.numel() // f.shape[-1], int(c), f.shape[-1])
                             for r, f, g, c in zip(reals, fakes, grads, c_reals)])
    d = dt(fakes[0])
    ws = workspace(int(A.lib().sgg_feature_match_workspace(pairs, L, d)), fakes[0].device)
    A.check(A.lib().sgg_feature_match(pairs, L, float(weight), _p(loss), _p(term), int(bool(accumulate_loss)), d, _p(ws), ws.numel(), _s()),
            "feature_match")
    return grads


def feature_match_ref(reals, fakes, c_reals, weight, loss=None, bf16=False):
    """The rule of ``feature_match`` in float64 NumPy (logging, tests):

        count_i = (elements of pair i) / Cpad_i * C_real_i;   m_i = sum over c < C_real_i of |fake_i - real_i| / count_i
        term = (m_0 + m_1 + ...) / L;   loss' = float32(weight * term) (+ loss, added in float32)
        grad_i = float32(weight / (L * count_i)) * sign(fake_i - real_i), 0 in padded channels, rounded to bfloat16 when ``bf16``

    ``weight`` enters as the f32 value the kernel receives; the sums are float64 in NumPy's order, not the kernel's
    (its chunk order is emulated by the tests).  Returns (float32 term, float32 loss, [float32 grad_i])."""
    f = np.float32
    w = float(f(weight))
    L = len(fakes)
    means, grads = [], []
    for r, x, c in zip(reals, fakes, c_reals):
        r, x = np.asarray(r, dtype=np.float64), np.asarray(x, dtype=np.float64)
        d = (x - r)[..., :int(c)]
        count = d.size
        means.append(float(np.abs(d).sum()) / count)
        g = np.zeros(x.shape, dtype=np.float32)
        g[..., :int(c)] = f(w / (L * count)) * np.sign(d).astype(np.float32)
        grads.append(torch.from_numpy(g).to(torch.bfloat16).to(torch.float32).numpy() if bf16 else g)
    term = 0.0
    for m in means:
        term += m
    term /= L
    out = f(w * term)
    return f(term), (out if loss is None else f(f(loss) + out)), grads


# ----------------------------------------------------------------------------- sliced Wasserstein distance (csrc/swd.hip)
SWD_K = 147                     # values of a descriptor: a 7x7 patch of three channels, (channel, y, x)
SWD_CHUNK = 256                  # descriptor rows per partial sum of the statistics (SW_CHUNK, csrc/swd.hip)
SWD_MAX_LEVELS = 5


def swd_default_levels(H, W):
    """The largest L <= 5 for which H and W divide by 2^(L-1) and min(H, W) >> (L-1) >= 16 (5 at 512x256, 4 at 128x128);
    0 where even one level is too small."""
    best = 0
    for L in range(1, SWD_MAX_LEVELS + 1):
        if H % (1 << (L - 1)) == 0 and W % (1 << (L - 1)) == 0 and (min(H, W) >> (L - 1)) >= 16:
            best = L
    return best


def swd_pyramid_elems(H, W, levels):
    """float32 values of one image's pyramid (levels concatenated, each [3][H >> l][W >> l]); 0: the shape is not supported."""
    return int(A.lib().sgg_swd_pyramid_elems(int(H), int(W), int(levels)))


def swd_pyramid(img, levels, out=None):
    """sgg_swd_pyramid: a device image (N,H,W,Cs), f32 / bf16 (Cs >= 3, values in [-1,1]) or uint8 (Cs = 3 | 4) -> the Laplacian
    pyramids (N, swd_pyramid_elems(H, W, levels)) float32 of its 8-bit colours.  2 * levels launches, no sync."""
    img, kind = _pixel_input(img)
    N, H, W, Cs = img.shape
    E = swd_pyramid_elems(H, W, levels)
    if E == 0:
        A.check(A.EUNSUPPORTED, f"swd_pyramid {H}x{W}, {levels} levels")
    out = _out(out, (N, E), torch.float32, img.device)
    need = int(A.lib().sgg_swd_pyramid_workspace(N, H, W, int(levels)))
    ws = workspace(need, img.device)
    A.check(A.lib().sgg_swd_pyramid(_p(img), kind, Cs, N, H, W, int(levels), _p(out), _p(ws), ws.numel(), _s()), "swd_pyramid")
    return out


def swd_descriptors(pyr, H, W, levels, level, patches, seed, image_offset, desc):
    """sgg_swd_descriptors: the pyramids (N, E) of images image_offset .. image_offset + N -> rows [i * patches + p] of ``desc``
    (a contiguous (N * patches, 147) float32 slice of the set-wide buffer).  One launch."""
    N = pyr.shape[0]
    assert pyr.dtype == torch.float32 and pyr.shape[1] == swd_pyramid_elems(H, W, levels)
    assert desc.dtype == torch.float32 and tuple(desc.shape) == (N * patches, SWD_K)
    A.check(A.lib().sgg_swd_descriptors(_p(pyr), N, int(H), int(W), int(levels), int(level), int(patches), int(seed) & 0xffffffff,
                                        int(image_offset), _p(desc), _s()), "swd_descriptors")
    return desc


def swd_project(desc, dirs, proj=None, moments=None):
    """sgg_swd_project: desc (M,147) float32, dirs (147,D) float32 -> (proj (D,M) float64, moments (3,2) float64 = per channel
    mean and population standard deviation).  Five launches, no sync."""
    M, D = desc.shape[0], dirs.shape[1]
    assert desc.dtype == torch.float32 and desc.shape[1] == SWD_K and dirs.dtype == torch.float32 and dirs.shape[0] == SWD_K
    proj = _out(proj, (D, M), torch.float64, desc.device)
    moments = _out(moments, (3, 2), torch.float64, desc.device)
    ws = workspace(int(A.lib().sgg_swd_project_workspace(M)), desc.device)
    A.check(A.lib().sgg_swd_project(_p(desc), M, _p(dirs), D, _p(proj), _p(moments), _p(ws), ws.numel(), _s()), "swd_project")
    return proj, moments


def swd_distance(sa, sb, out=None):
    """sgg_swd_distance: two (D,M) float64 tensors with sorted rows -> out[d] = sum_m |sa[d][m] - sb[d][m]|, float64 (D,)."""
    D, M = sa.shape
    assert sa.dtype == torch.float64 and sb.dtype == torch.float64 and tuple(sb.shape) == (D, M)
    out = _out(out, (D,), torch.float64, sa.device)
    A.check(A.lib().sgg_swd_distance(_p(sa), _p(sb), D, M, _p(out), _s()), "swd_distance")
    return out
