"""Bit-exact parity of the FUSED and TWO-NETWORK forms of the conv forward / data gradient at the edge rows of
tests/conv_edge_cases.py -- the entry points a training step calls instead of the plain ones test_gpu_conv_edges.py pins:
the statistics epilogues (conv_fwd_stats, deconv_fwd_stats), the norm-backward sums and the mixed-precision result of the data
gradient, the paired forms, normalise on load, and the grouped (group2) calls.

Same technique as test_gpu_conv_edges.py: integer operands, so every result -- the statistics rows included: integer sums
below 2^24, exact in f32 in any order -- equals the float64 oracle element for element, with no tolerance.  Every case asserts
the route and the eligibility its row is pinned to first, writes every result into sentinel guard cells (statistics buffers
pre-filled with NaN: an unwritten row is seen) and checks the cells afterwards.  The two-network forms run network A (the
row's draw) beside an independent network B, each half compared with its own oracle: a swapped weight, bias or batch offset
changes values.  The chunk-to-pixel mapping of the statistics rows is not part of the ABI; their sum over the chunks is."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import conv_edge_cases as E

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
dev, padc, Guarded = E.dev, E.padc, E.Guarded


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    import sggan_amd.kernels  # noqa: F401
    return sggan_amd


def pinned(row, dtype):
    """The row's route and eligibility on this device's library: a lab build or a config difference cannot hide a moved shape."""
    g = E.geom(row, dtype)
    assert E.routes(g) == E.row_routes(row, dtype), (row[0], dtype)
    assert E.eligible(g) == E.row_eligible(row, dtype), (row[0], dtype)


def nan_rows(shape):
    return Guarded(shape, F32, fill=float("nan"))


def stats_same(part, exp, what):
    """No row left unwritten, and the rows summed over their chunks (float64 on the host side of the comparison) equal the oracle's."""
    assert not bool(torch.isnan(part.t).any()), f"{what}: a statistics row was not written"
    E.same(part.t.to(torch.float64).sum(1), exp, what)
    part.check(what)


def acts():
    from sggan_amd import _abi as A
    return ((A.ACT_NONE, 0.0, "none"), (A.ACT_RELU, 0.0, "relu"), (A.ACT_LRELU, 0.5, "lrelu"))


# ---------------------------------------------------------------------------------------------------- a. forward statistics epilogue
@pytest.mark.parametrize("name", E.STATS_FWD)
def test_forward_statistics_epilogue_bit_exact(sg, name):
    K = sg.kernels
    row = E.BY_NAME[name]
    pinned(row, "bf16")
    e = E.expected(name)
    g, x, _, wf, _, b = E.operands(sg, row, "bf16", e)
    assert g.stats_chunks > 0
    yc = g.y_shape[3]
    y, part = Guarded(g.y_shape, BF), nan_rows((g.y_shape[0], g.stats_chunks, yc, 2))
    K.conv_fwd_stats(g, x, wf, b, out=y.t, out_partial=part.t)
    ys = E.store(padc(e.y, yc), BF)
    E.same(y.t, ys, f"{name} y")
    y.check(f"{name} y")
    stats_same(part, E.stat_sums(ys), f"{name} (sum y, sum y^2)")


# ---------------------------------------------------------------------------------------------------- b. data gradient + norm-backward sums
def norm_operands(name, g):
    c = E.norm_bwd_case(name)
    assert c.nx.shape == g.x_shape                       # (these rows' channel counts are multiples of 8: nothing to pad)
    return c, dev(c.nx, BF), dev(c.stats), dev(c.gamma), dev(c.beta)


@pytest.mark.parametrize("name", E.STATS_BWD)
def test_data_gradient_norm_backward_sums_bit_exact(sg, name):
    from sggan_amd import _abi as A
    K = sg.kernels
    row = E.BY_NAME[name]
    pinned(row, "bf16")
    e = E.expected(name)
    g, _, dy, _, wd, _ = E.operands(sg, row, "bf16", e)
    assert g.bwd_stats_chunks > 0
    c, nx, st, gam, bet = norm_operands(name, g)
    add = E.addend(name, e.x.shape)
    pshape = (g.x_shape[0], g.bwd_stats_chunks, g.x_shape[3], 2)
    for addend in (None, add):
        dxs = E.store(e.dx + (0.0 if addend is None else addend), BF)
        for act, leak, an in acts():
            tag = f"{name} addend={addend is not None} act={an}"
            dx, part = Guarded(g.x_shape, BF), nan_rows(pshape)
            K.conv_dgrad_stats(g, dy, wd, None if addend is None else dev(addend, BF), nx, st, gam, bet, act, leak, out=dx.t, out_partial=part.t)
            E.same(dx.t, dxs, tag + " dx")
            dx.check(tag + " dx")
            stats_same(part, E.norm_bwd_sums(dxs, c, an, leak), tag + " (sum g, sum g xhat)")
    dx, part = Guarded(g.x_shape, BF), Guarded(pshape, F32)
    with pytest.raises(A.SggError, match=rf"\({A.EUNSUPPORTED}\)"):
        K.conv_dgrad_stats(g, dy, wd, None, nx, st, gam, bet, A.ACT_TANH, 0.0, out=dx.t, out_partial=part.t)
    dx.untouched(f"{name} tanh dx")
    part.untouched(f"{name} tanh partial")


# ---------------------------------------------------------------------------------------------------- c. mixed precision
@pytest.mark.parametrize("name", E.STATS_BWD)
def test_mixed_precision_data_gradient_bit_exact(sg, name):
    """bf16 operands, f32 result: with an f32 addend of odd integers around +-1001 (bf16 holds none of them) the sum is exact only
    if neither the result nor the addend passes through bf16."""
    K = sg.kernels
    row = E.BY_NAME[name]
    pinned(row, "bf16")
    e = E.expected(name)
    g, _, dy, _, wd, _ = E.operands(sg, row, "bf16", e)
    assert g.dgrad_mixed
    big = E.addend_f32(name, e.x.shape)
    assert np.array_equal(E.store(big, F32), big) and not np.array_equal(E.store(big, BF), big)
    for an, addend, adt in (("none", None, None), ("bf16", E.addend(name, e.x.shape), BF), ("f32", big, F32)):
        dx = Guarded(g.x_shape, F32)
        out = K.conv_dgrad(g, dy, wd, None if addend is None else dev(addend, adt), out_f32=True, out=dx.t)
        assert out.data_ptr() == dx.t.data_ptr() and out.dtype == F32
        E.same(dx.t, e.dx + (0.0 if addend is None else addend), f"{name} f32 dx, addend {an}")
        dx.check(f"{name} f32 dx, addend {an}")


# ---------------------------------------------------------------------------------------------------- d. paired forms
def paired_operands(sg, name, nsplit):
    """The stacked batch of a paired form: geometry at the stacked size, A's and B's packed weights and biases."""
    K = sg.kernels
    row = E.BY_NAME[name]
    ea, eb = E.expected(name), E.expected_b(name)
    n = 2 if row[7] == 1 else row[7]
    g = E.geom_n(row, "bf16", n)
    pinned(row, "bf16")
    xc, yc = g.x_shape[3], g.y_shape[3]
    pk = (lambda e: K.pack_weights(dev(e.w), yc, xc, BF)) if g.is_deconv else (lambda e: K.pack_weights(dev(e.w), xc, yc, BF))
    t = lambda field, cp: padc(E.paired(name, nsplit, field), cp)        # noqa: E731
    return g, t("x", xc), t("y", yc), t("dy", yc), t("dx", xc), pk(ea), pk(eb), dev(padc(ea.b, yc)), dev(padc(eb.b, yc))


@pytest.mark.parametrize("name,nsplit", E.PAIRED, ids=[f"{n}-nsplit{k}" for n, k in E.PAIRED])
def test_paired_forward_and_data_gradient_bit_exact(sg, name, nsplit):
    from sggan_amd import _abi as A
    K = sg.kernels
    g, x, ye, dy, dxe, (wfa, wda), (wfb, wdb), ba, bb = paired_operands(sg, name, nsplit)
    assert g.pair_ok and g.stats_chunks > 0 and E.routes(g)[:2] == ("HALO3", "HALO3") and 0 < nsplit < g.x_shape[0]
    tag = f"{name} nsplit {nsplit}"
    xt, dyt = dev(x, BF), dev(dy, BF)
    pshape = (g.y_shape[0], g.stats_chunks, g.y_shape[3], 2)
    y, part = Guarded(g.y_shape, BF), nan_rows(pshape)
    K.conv_fwd_stats_pair(g, xt, wfa, ba, wfb, bb, nsplit, out=y.t, out_partial=part.t)
    ys = E.store(ye, BF)
    E.same(y.t, ys, tag + " y")
    y.check(tag + " y")
    stats_same(part, E.stat_sums(ys), tag + " (sum y, sum y^2)")
    add = padc(E.addend(name, x.shape[:3] + (E.BY_NAME[name][5],)), g.x_shape[3])
    for addend in (None, add):                           # (REFLECT: through the folded side tensor)
        dx = Guarded(g.x_shape, BF)
        K.conv_dgrad_pair(g, dyt, wda, wdb, nsplit, None if addend is None else dev(addend, BF), out=dx.t)
        E.same(dx.t, E.store(dxe + (0.0 if addend is None else addend), BF), f"{tag} dx addend={addend is not None}")
        dx.check(f"{tag} dx addend={addend is not None}")
    # nsplit 0 and N: refused on the host (sgg_conv2d_fwd_stats_pair / sgg_conv2d_bwd_data_pair check it before anything is launched)
    L, p, s = A.lib(), K._p, K._s
    ws = K.workspace(max(g.ws_fwd, g.ws_dgrad, 1), "cuda")
    for bad in (0, g.x_shape[0]):
        y, part, dx = Guarded(g.y_shape, BF), Guarded(pshape, F32), Guarded(g.x_shape, BF)
        assert L.sgg_conv2d_fwd_stats_pair(C.byref(g.desc), p(xt), p(wfa), p(ba), p(wfb), p(bb), bad, p(y.t), p(part.t), p(ws), ws.numel(), s()) == A.EINVAL
        assert L.sgg_conv2d_bwd_data_pair(C.byref(g.desc), p(dyt), p(wda), p(wdb), bad, None, p(dx.t), p(ws), ws.numel(), s()) == A.EINVAL
        for t, what in ((y, "y"), (part, "partial"), (dx, "dx")):
            t.untouched(f"{tag} {what} with nsplit {bad}")


# ---------------------------------------------------------------------------------------------------- e. normalise on load
@pytest.mark.parametrize("name,nsplit", E.NORMLOAD, ids=[f"{n}-nsplit{k}" for n, k in E.NORMLOAD])
def test_normalise_on_load_bit_exact(sg, name, nsplit):
    K = sg.kernels
    row = E.BY_NAME[name]
    pinned(row, "bf16")
    ea, eb = E.expected(name), E.expected_b(name)
    g, _, _, wfa, _, ba = E.operands(sg, row, "bf16", ea)
    assert g.normload_ok and g.stats_chunks > 0 and (nsplit == 0 or (g.pair_ok and 0 < nsplit < g.x_shape[0]))
    c = E.normload_case(name)
    assert c.x_raw.shape == g.x_shape
    if nsplit:
        wfb, _ = K.pack_weights(dev(eb.w), g.x_shape[3], g.y_shape[3], BF)
        pair = (dev(c.gamma[1]), dev(c.beta[1]), wfb, dev(padc(eb.b, g.y_shape[3])), nsplit)
        xn, ye = E.mix(c.x_norm[0], c.x_norm[1], nsplit), E.mix(c.y[0], c.y[1], nsplit)
    else:
        pair, xn, ye = None, c.x_norm[0], c.y[0]
    tag = f"{name} nsplit {nsplit}"
    xo, y, part = Guarded(g.x_shape, BF), Guarded(g.y_shape, BF), nan_rows((g.y_shape[0], g.stats_chunks, g.y_shape[3], 2))
    K.conv_fwd_stats_normload(g, dev(c.x_raw, BF), dev(c.stats), dev(c.gamma[0]), dev(c.beta[0]), wfa, ba, pair,
                              out=y.t, out_partial=part.t, out_norm=xo.t)
    E.same(xo.t, xn, tag + " x_norm")
    xo.check(tag + " x_norm")
    ys = E.store(padc(ye, g.y_shape[3]), BF)
    E.same(y.t, ys, tag + " y")
    y.check(tag + " y")
    stats_same(part, E.stat_sums(ys), tag + " (sum y, sum y^2)")


def test_normalise_on_load_stops_at_its_table(sg):
    """halo3_normload_out_c576: one 64-channel chunk past the kernel's table of per-channel constants.  The shape keeps the
    statistics epilogue and loses this form: the query says so and the entry point returns the unsupported error on the host."""
    from sggan_amd import _abi as A
    K = sg.kernels
    row = E.BY_NAME["halo3_normload_out_c576"]
    pinned(row, "bf16")
    e = E.expected(row[0])
    g, x, _, wf, _, b = E.operands(sg, row, "bf16", e)
    assert not g.normload_ok and g.stats_chunks > 0 and g.x_shape[3] == 576
    N, Cn = g.x_shape[0], g.x_shape[3]
    st = torch.ones((N, Cn, 2), device="cuda")
    gam, bet = torch.ones(Cn, device="cuda"), torch.zeros(Cn, device="cuda")
    xo, y, part = Guarded(g.x_shape, BF), Guarded(g.y_shape, BF), Guarded((N, g.stats_chunks, g.y_shape[3], 2), F32)
    p = K._p
    rc = A.lib().sgg_conv2d_fwd_stats_normload(C.byref(g.desc), p(x), p(st), p(gam), p(bet), None, None, p(xo.t), p(wf), p(b), None, None, 0,
                                               p(y.t), p(part.t), None, 0, K._s())
    assert rc == A.EUNSUPPORTED
    for t, what in ((xo, "x_norm"), (y, "y"), (part, "partial")):
        t.untouched(f"{row[0]} {what}")


# ---------------------------------------------------------------------------------------------------- f. transposed conv with statistics
@pytest.mark.parametrize("name,nsplit", E.DECONV_STATS, ids=[f"{n}-nsplit{k}" for n, k in E.DECONV_STATS])
def test_transposed_conv_statistics_bit_exact(sg, name, nsplit):
    K = sg.kernels
    row = E.BY_NAME[name]
    tag = f"{name} nsplit {nsplit}"
    if nsplit:
        g, x, ye, _, _, (_, wda), (_, wdb), ba, bb = paired_operands(sg, name, nsplit)
        pair = (wdb, bb, nsplit)
        assert 0 < nsplit < g.x_shape[0]
    else:
        pinned(row, "bf16")
        e = E.expected(name)
        g, xt, _, _, wda, ba = E.operands(sg, row, "bf16", e)
        x, ye, pair = xt, padc(e.y, g.y_shape[3]), None
    assert g.is_deconv and g.stats_chunks == E.row_eligible(row, "bf16")[0] > 0 and E.routes(g)[0] == "S2HALO"
    y, part = Guarded(g.y_shape, BF), nan_rows((g.y_shape[0], g.stats_chunks, g.y_shape[3], 2))
    K.deconv_fwd_stats(g, x if nsplit == 0 else dev(x, BF), wda, ba, pair, out=y.t, out_partial=part.t)
    ys = E.store(ye, BF)
    E.same(y.t, ys, tag + " y")
    y.check(tag + " y")
    stats_same(part, E.stat_sums(ys), tag + " (sum y, sum y^2)")


# ---------------------------------------------------------------------------------------------------- g. grouped two-network calls
# The grp == 2 path a row is there for: (0 forward | 1 data gradient, the route that reaches it, the dtypes it holds in)
REACHES = {
    "glds_256x256_fwd_ragged": (0, "GLDS_256x256", ("bf16", "f32")), "glds_256x128_3stage": (0, "GLDS_256x128", ("bf16", "f32")),
    "glds_128x128_long_k": (0, "GLDS_128x128", ("bf16", "f32")), "glds_256x256_dgrad_s2": (1, "GLDS_256x256", ("bf16", "f32")),
    "splitk_fwd_dc40": (0, "GLDS_128x64+SPLITK", ("bf16", "f32")), "splitk_dgrad_dc40": (1, "GLDS_128x64+SPLITK", ("bf16", "f32")),
    "splitk_fwd_dc264": (0, "GLDS_128x128+SPLITK", ("bf16", "f32")), "splitk_dgrad_dc264": (1, "GLDS_128x128+SPLITK", ("bf16", "f32")),
    "pointwise_c512": (0, "GLDS_128x128+SPLITK", ("f32",)),
    "halo3_min_same": (0, "HALO3", ("bf16",)), "halo3_n3_dtail_same": (0, "HALO3", ("bf16",)),
    "halo3_n3_dtail_reflect": (0, "HALO3", ("bf16",)), "halo3_dgrad_dtail_reflect": (1, "HALO3", ("bf16",)),
    "s2halo_min": (1, "S2HALO", ("bf16",)), "s2halo_min_deconv": (0, "S2HALO", ("bf16",)), "s2halo_deconv_n3": (0, "S2HALO", ("bf16",)),
    "s2n_wo5": (1, "S2N", ("bf16",)), "s2n_wo130": (1, "S2N", ("bf16",)),
    "head7_ragged": (0, "N7", ("bf16",)), "head7_16x32": (1, "HALO_NARROW_IN", ("bf16", "f32")), "stem7_16x32": (0, "HALO_NARROW_IN", ("bf16", "f32")),
    "stem7_17x33": (1, "N7", ("bf16",)), "narrow5_16x32": (0, "HALO_FWD", ("bf16", "f32")),
    "narrow5_in16_16x32": (1, "HALO_DGRAD_NARROW", ("bf16", "f32")), "narrow5_in16_reflect": (1, "HALO_DGRAD_NARROW", ("bf16", "f32")),
    "deconv_ragged": (0, "GLDS_128x64", ("bf16", "f32")), "wgrad_128x64_cr3": (0, "GLDS_128x64", ("bf16", "f32")),
    # stride-1 transposed convs: deconv_fwd_group2 is the stacked halo launch in the data-gradient direction with bias / bias2 picked per
    # image (no conv-side form passes a bias there), deconv_dgrad_group2 the stacked forward direction without one
    "tconv1_halo3_pair_n3": (0, "HALO3", ("bf16",)), "tconv1_halo3_c512": (0, "HALO3", ("bf16",)), "tconv1_halo3_n3_dtail": (0, "HALO3", ("bf16",)),
    "tconv1_halo3_src264": (1, "HALO3", ("bf16",)), "tconv1_head_c3": (0, "HALO3", ("bf16",)),
    "tconv1_splitk": (0, "GLDS_128x128+SPLITK", ("bf16", "f32")), "tconv1_ragged": (0, "GLDS_128x64", ("bf16", "f32")),
}
# How the grouped forward / data gradient of the transposed rows run in bf16 (plan_conv's `group`, from the route): the halo kernel
# picks weights and bias per image, so its grouped call is the single launch on 2N images split at N; the generic GEMM doubles its grid.
TCONV1_GROUP = {
    "tconv1_halo3_pair_n3": ("stacked", "stacked"), "tconv1_halo3_c512": ("stacked", "stacked"), "tconv1_halo3_n3_dtail": ("stacked", "one launch"),
    "tconv1_halo3_src264": ("one launch", "stacked"), "tconv1_head_c3": ("stacked", "one launch"), "tconv1_splitk": ("one launch", "one launch"),
    "tconv1_ragged": ("one launch", "one launch"),
}


def group_path(route):
    return "stacked" if route in ("HALO3", "S2HALO") else "one launch" if route.startswith("GLDS_") else "two calls"


def group2_operands(sg, row, dtype):
    K = sg.kernels
    ea, eb = E.expected(row[0]), E.expected_b(row[0])
    g, xa, dya, wfa, wda, ba = E.operands(sg, row, dtype, ea)
    _, xb, dyb, wfb, wdb, bb = E.operands(sg, row, dtype, eb)
    return K, ea, eb, g, torch.cat([xa, xb]), torch.cat([dya, dyb]), (wfa, wda, ba), (wfb, wdb, bb)


@pytest.mark.parametrize("row,dtype", E.GROUP2_CASES, ids=[f"{r[0]}-{dt}" for r, dt in E.GROUP2_CASES])
def test_grouped_two_network_calls_bit_exact(sg, row, dtype):
    name = row[0]
    dt = E.DTYPES[dtype]
    pinned(row, dtype)
    op, route, dts = REACHES[name]
    K, ea, eb, g, x, dy, (wfa, wda, ba), (wfb, wdb, bb) = group2_operands(sg, row, dtype)
    if dtype in dts:
        assert E.routes(g)[op] == route, (name, dtype, E.routes(g))
    if name in TCONV1_GROUP and dtype == "bf16":
        assert g.is_deconv and tuple(group_path(r) for r in E.routes(g)[:2]) == TCONV1_GROUP[name], (name, E.routes(g))
    for r, ws in zip(E.routes(g)[:2], (g.ws_fwd, g.ws_dgrad)):
        assert not r.endswith("+SPLITK") or ws > 0       # split K: the grouped call needs, and the launcher passes, twice this
    tag = f"{name}[{dtype}] {E.routes(g)[:2]}"
    xc, yc = g.x_shape[3], g.y_shape[3]
    N = g.x_shape[0]
    # forward, three activations
    ye = np.concatenate([padc(ea.y, yc), padc(eb.y, yc)])
    for act, leak, an in acts():
        f = {"none": lambda v: v, "relu": lambda v: np.maximum(v, 0.0), "lrelu": lambda v: np.where(v > 0, v, 0.5 * v)}[an]
        y = Guarded((2 * N,) + tuple(g.y_shape[1:]), dt)
        if g.is_deconv:
            K.deconv_fwd_group2(g, x, wda, ba, wdb, bb, act, leak, out=y.t)
        else:
            K.conv_fwd_group2(g, x, wfa, ba, wfb, bb, act, leak, out=y.t)
        E.same(y.t, E.store(f(ye), dt), f"{tag} group2 y act {an}")
        y.check(f"{tag} group2 y act {an}")
    # data gradient, plain and (conv) with an addend
    dxe = np.concatenate([padc(ea.dx, xc), padc(eb.dx, xc)])
    add = padc(E.addend(name, (2 * N,) + ea.x.shape[1:]), xc)
    for addend in (None,) if g.is_deconv else (None, add):
        dx = Guarded((2 * N,) + tuple(g.x_shape[1:]), dt)
        if g.is_deconv:
            K.deconv_dgrad_group2(g, dy, wfa, wfb, out=dx.t)
        else:
            K.conv_dgrad_group2(g, dy, wda, wdb, None if addend is None else dev(addend, dt), out=dx.t)
        E.same(dx.t, E.store(dxe + (0.0 if addend is None else addend), dt), f"{tag} group2 dx addend={addend is not None}")
        dx.check(f"{tag} group2 dx addend={addend is not None}")
    # bias gradient of the two halves
    for accumulate in (False, True):
        dba, dbb = Guarded(ea.db.shape, F32, fill=5.0), Guarded(eb.db.shape, F32, fill=-3.0)
        K.bias_grad_group2(dy, dba.t, dbb.t, accumulate=accumulate)
        E.same(dba.t, ea.db + (5.0 if accumulate else 0.0), f"{tag} group2 dbA accumulate={accumulate}")
        E.same(dbb.t, eb.db + (-3.0 if accumulate else 0.0), f"{tag} group2 dbB accumulate={accumulate}")
        dba.check(f"{tag} group2 dbA")
        dbb.check(f"{tag} group2 dbB")


def test_lockstep_head_writes_into_a_batch_slice_of_a_larger_tensor(sg):
    """tconv1_head_c3 (d8: 64 -> 3, 8 stored channels), stacked forward through out=: the 2N = 6 images go into images 2..7 of a guarded
    tensor of 10 -- what the lockstep U-Net's d8 does with the discriminators' stacked input.  The images before and after the slice
    keep their sentinel bytes, like the cells around the tensor."""
    row = E.BY_NAME["tconv1_head_c3"]
    pinned(row, "bf16")
    K, ea, eb, g, x, _, (_, wda, ba), (_, wdb, bb) = group2_operands(sg, row, "bf16")
    assert g.is_deconv and E.routes(g)[0] == "HALO3" and g.y_shape == (3, 6, 256, 8)
    ye = np.concatenate([padc(ea.y, 8), padc(eb.y, 8)])
    for act, leak, an in acts():
        f = {"none": lambda v: v, "relu": lambda v: np.maximum(v, 0.0), "lrelu": lambda v: np.where(v > 0, v, 0.5 * v)}[an]
        big = Guarded((10,) + tuple(g.y_shape[1:]), BF)
        out = K.deconv_fwd_group2(g, x, wda, ba, wdb, bb, act, leak, out=big.t[2:8])
        assert out.data_ptr() == big.t[2].data_ptr()
        E.same(big.t[2:8], E.store(f(ye), BF), f"tconv1_head_c3 group2 y into a slice, act {an}")
        big.check(f"tconv1_head_c3 group2 y into a slice, act {an}")
        for lo, hi in ((0, 2), (8, 10)):
            assert bool((big.t[lo:hi].contiguous().view(torch.uint8) == 0xA5).all()), f"act {an}: images {lo}..{hi - 1} beside the slice were written"


def test_stride1_transposed_conv_has_no_statistics_epilogue(sg):
    """tconv1_halo3_pair_n3 runs HALO3 in both directions, and still sgg_deconv2d_fwd_stats has no form for it, single or stacked
    (the statistics epilogue of a transposed conv is the stride-2 kernel's): unsupported, before anything is launched."""
    from sggan_amd import _abi as A
    row = E.BY_NAME["tconv1_halo3_pair_n3"]
    pinned(row, "bf16")
    K, _, _, g, x, _, (_, wda, ba), (_, wdb, bb) = group2_operands(sg, row, "bf16")
    assert g.is_deconv and g.stats_chunks == 0 and not g.pair_ok and E.routes(g)[:2] == ("HALO3", "HALO3")
    p = K._p
    xa = x[:g.x_shape[0]].contiguous()
    for w2, b2, nsplit in ((None, None, 0), (wdb, bb, 1)):
        y, part = Guarded(g.y_shape, BF), Guarded((g.y_shape[0], 4, g.y_shape[3], 2), F32)
        rc = A.lib().sgg_deconv2d_fwd_stats(C.byref(g.desc), p(xa), p(wda), p(ba), p(w2), p(b2), nsplit, p(y.t), p(part.t), None, 0, K._s())
        assert rc == A.EUNSUPPORTED
        y.untouched(f"{row[0]} y, nsplit {nsplit}")
        part.untouched(f"{row[0]} partial, nsplit {nsplit}")


def test_grouped_split_k_call_refuses_the_single_workspace(sg):
    """splitk_fwd_dc40: the grouped call splits K for each network into slabs of its own and needs twice the single call's
    workspace; with the single call's size run_conv returns the workspace error before anything is launched."""
    from sggan_amd import _abi as A
    row = E.BY_NAME["splitk_fwd_dc40"]
    K, _, _, g, x, _, (wfa, _, ba), (wfb, _, bb) = group2_operands(sg, row, "bf16")
    assert E.routes(g)[0].endswith("+SPLITK") and g.ws_fwd > 0
    ws = K.workspace(2 * g.ws_fwd, "cuda")
    y = Guarded((2 * g.y_shape[0],) + tuple(g.y_shape[1:]), BF)
    p = K._p
    rc = A.lib().sgg_conv2d_fwd_group2(C.byref(g.desc), p(x), p(wfa), p(ba), p(wfb), p(bb), p(y.t), A.ACT_NONE, 0.0, p(ws), g.ws_fwd, K._s())
    assert rc == A.EWORKSPACE
    y.untouched("splitk_fwd_dc40 group2 y with the single call's workspace")


def test_short_workspace_is_refused_before_the_fold_gather(sg):
    """halo3_n3_dtail_reflect: a REFLECT data gradient on the split-K GEMM, so its workspace has both parts, the pre-folded
    gather rows of the border pixels and behind them the slabs.  A workspace that holds the first part and not all of the second
    is refused before anything is launched: the fold gather, the call's first launch, has not written into it."""
    from sggan_amd import _abi as A
    row = E.BY_NAME["halo3_n3_dtail_reflect"]
    pinned(row, "bf16")
    e = E.expected(row[0])
    g, _, dy, _, wd, _ = E.operands(sg, row, "bf16", e)
    d = g.desc
    assert E.routes(g)[1] == "GLDS_128x64+SPLITK" and (d.N, d.H, d.W, d.C, d.K) == (3, 6, 256, 64, 264) and d.pad_mode == A.PAD_REFLECT
    border = 2 * d.pad_t * d.W + (d.H - 2 * d.pad_t) * 2 * d.pad_t           # the 2p border rows, then the 2p border columns of the rest
    fold = -(-(d.N * border * d.R * d.S * d.K * 2) // 256) * 256
    assert g.ws_dgrad > fold + 256                       # the short workspace below still covers the fold part
    K = sg.kernels
    ws = torch.full((g.ws_dgrad,), 0x5A, dtype=torch.uint8, device="cuda")
    dx = Guarded(g.x_shape, BF)
    rc = A.lib().sgg_conv2d_bwd_data(C.byref(d), K._p(dy), K._p(wd), None, K._p(dx.t), K._p(ws), g.ws_dgrad - 256, K._s())
    assert rc == A.EWORKSPACE
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all()), "the workspace was written before it was found too short"
    dx.untouched("halo3_n3_dtail_reflect dx with a short workspace")
