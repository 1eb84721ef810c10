"""The ONE rounding of every conv epilogue, at the edge rows of tests/conv_edge_cases.py.

test_gpu_conv_edges.py and test_gpu_conv_fused_edges.py use operands from {-1, 0, 1}, chosen so that no rounding rule enters: they
say where every value goes and nothing about how an epilogue turns its f32 accumulator into the stored value.  Here x and dy stay in
{-1, 0, 1} and the weights, the bias and the addend carry fraction bits (conv_edge_cases.rounding: k/128 in bf16, k/4096 in f32), with
sum |terms| 2^f < 2^24 per output element: the f32 accumulation is exact in any order and split, the float64 oracle is exact, and the
stored value must be ONE round-to-nearest-even of it -- store().  Half to all of the elements need that rounding, so an epilogue that
truncates, rounds before it adds the bias / applies the activation / joins the addend, passes its split-K slabs through bf16, sums
the accumulator instead of the stored output into its statistics rows, or (f32 rows: compared with no rounding at all) feeds its
MFMA operands at reduced precision differs in a tenth to all of the elements (test_conv_edges_cpu.py asserts those shares on the
oracle alone).  LeakyReLU runs at the discriminators' leak 0.2, not exact in binary; tanh against the library's own f32 tanh kernel on
the exact pre-activation, rounded once.

One documented exception: the bf16 REFLECT data gradient behind HALO_NARROW_IN / HALO_DGRAD_NARROW rounds twice on the band the
mirrored terms reach (conv_border_fold_kernel reads the stored dx); E.fold_two_step is that value, asserted exactly.

Every case asserts the route and the eligibility its row is pinned to first and writes into sentinel guard cells."""
import numpy as np
import pytest
import torch

from tests import conv_edge_cases as E
from tests.test_gpu_conv_edges import FUSED

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
dev, padc, Guarded = E.dev, E.padc, E.Guarded
LEAK = 0.2                                               # the discriminators' LeakyReLU

# a, b: the FUSED rows of test_gpu_conv_edges.py, the long-reduction in-kernel epilogue and the two border-fold rows
ROWS_AB = FUSED + ["glds_128x128_long_k"] + E.FOLD_TWICE
CASES_AB = [(E.BY_NAME[n], dt) for n in ROWS_AB for dt in E.BY_NAME[n][10]]
IDS_AB = [f"{r[0]}-{dt}" for r, dt in CASES_AB]
TANH_ROUTES = ("N7", "HALO_FWD")
TANH_ROWS = ("glds_128x128_long_k", "splitk_fwd_dc40", "s2halo_min_deconv",
             "tconv1_head_c3", "tconv1_halo3_min")       # d8's own activation: HALO3 at 8 destination channels (f32: behind the split-K reduce), and at 64
# the stacked forward of two networks (deconv_fwd_group2), each with a fractional draw of its own
GROUPED_FWD = ["tconv1_halo3_pair_n3"]
# d: the f32 rows of FUSED; left out: rows whose weight-gradient draw holds fewer than 9 fraction bits inside the exactness bound.
# None: the two rows with 2 x 101 x 103 = 20806 pixels per element of dw hold 11, every other row 12 (test_conv_edges_cpu.py asserts
# that the list is exactly the rows below 9).
WGRAD_ROWS = [n for n in FUSED if "f32" in E.BY_NAME[n][10]]
WGRAD_LEFT_OUT = ()
WGRAD_MIN_F = 9


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    import sggan_amd.kernels  # noqa: F401
    return sggan_amd


# Module-scoped parametrised fixtures: pytest runs the tests of one parameter next to each other, so a case's forward and data-gradient
# tests (and a STATS_BWD row's two tests) share one evaluation of E.rounding's small cache.
@pytest.fixture(scope="module", params=CASES_AB, ids=IDS_AB)
def case(request):
    return request.param


@pytest.fixture(scope="module", params=E.STATS_BWD)
def bwd_name(request):
    return request.param


def pinned(row, dtype):
    """The row's route and eligibility on this device's library: a lab build or a config difference cannot hide a moved shape."""
    g = E.geom(row, dtype)
    assert E.routes(g) == E.row_routes(row, dtype), (row[0], dtype)
    assert E.eligible(g) == E.row_eligible(row, dtype), (row[0], dtype)


def wants_tanh(row, dtype):
    return E.row_routes(row, dtype)[0] in TANH_ROUTES or row[0] in TANH_ROWS


# ---------------------------------------------------------------------------------------------------- a. forward, per route
def test_forward_epilogue_rounds_once(sg, case):
    row, dtype = case
    from sggan_amd import _abi as A
    from tests.test_gpu_small_kernels import close
    K = sg.kernels
    name = row[0]
    dt = E.DTYPES[dtype]
    pinned(row, dtype)
    e = E.rounding(name, dtype)
    g, x, _, wf, wd, b = E.operands(sg, row, dtype, e)
    tag = f"{name}[{dtype}] {E.routes(g)[0]}"
    fwd = (lambda act, leak, out: K.deconv_fwd(g, x, wd, b, act, leak, out=out)) if g.is_deconv else \
          (lambda act, leak, out: K.conv_fwd(g, x, wf, b, act, leak, out=out))
    pre = padc(e.y, g.y_shape[3])                        # the exact pre-activation, bias included; f32 holds it (the CPU suite's bound)
    if dtype == "f32":
        assert np.array_equal(E.store(pre, F32), pre)    # nothing is rounded: every difference is operand or accumulator precision
    for act, leak, exp in ((A.ACT_NONE, 0.0, pre), (A.ACT_RELU, 0.0, np.maximum(pre, 0.0)), (A.ACT_LRELU, LEAK, E.lrelu_f32(pre, LEAK))):
        y = Guarded(g.y_shape, dt)
        fwd(act, leak, y.t)
        E.same(y.t, E.store(exp, dt), f"{tag} y act {act}")
        y.check(f"{tag} y act {act}")
    if not wants_tanh(row, dtype):
        return
    # tanh: the library's own tanhf (sgg_act_fwd in f32) of the exact pre-activation, then the one rounding -- order and rounding
    # alone, compared exactly; and float64 tanh at the tolerance the activation kernel itself is held to
    ref = K.act_fwd(dev(pre, F32), A.ACT_TANH).to(dt)
    y = Guarded(g.y_shape, dt)
    fwd(A.ACT_TANH, 0.0, y.t)
    E.same(y.t, ref.to(torch.float64).cpu().numpy(), f"{tag} y tanh")
    y.check(f"{tag} y tanh")
    close(y.t, np.tanh(pre), dt, f"{tag} y tanh against float64")


# ---------------------------------------------------------------------------------------------------- b. data gradient
def test_data_gradient_epilogue_rounds_once(sg, case):
    row, dtype = case
    K = sg.kernels
    name = row[0]
    dt = E.DTYPES[dtype]
    pinned(row, dtype)
    e = E.rounding(name, dtype)
    g, _, dy, wf, wd, _ = E.operands(sg, row, dtype, e)
    tag = f"{name}[{dtype}] {E.routes(g)[1]}"
    xc = g.x_shape[3]
    dxp = padc(e.dx, xc)
    exp = E.store(dxp, dt)
    if dtype == "f32":
        assert np.array_equal(exp, dxp)
    elif name in E.FOLD_TWICE:                           # the documented second rounding on the fold's band
        assert E.routes(g)[1] in ("HALO_NARROW_IN", "HALO_DGRAD_NARROW") and row[4].startswith("REFLECT")
        band, two = E.fold_two_step(name)
        assert band.any() and (two != E.store(e.dx, dt))[band].any()
        exp = padc(two, xc)
    dx = Guarded(g.x_shape, dt)
    if g.is_deconv:
        K.deconv_dgrad(g, dy, wf, out=dx.t)
    else:
        K.conv_dgrad(g, dy, wd, out=dx.t)
    E.same(dx.t, exp, tag + " dx")
    dx.check(tag + " dx")
    if g.is_deconv:                                      # (the transposed conv has no addend form)
        return
    add = padc(E.frac_addend(name, e.x.shape, dtype), xc)
    dx = Guarded(g.x_shape, dt)
    K.conv_dgrad(g, dy, wd, dev(add, dt), out=dx.t)      # (an addend takes the narrow halo routes' shapes to the generic GEMM: one rounding)
    E.same(dx.t, E.store(dxp + add, dt), tag + " dx + addend")
    dx.check(tag + " dx + addend")


@pytest.mark.parametrize("name", GROUPED_FWD)
def test_grouped_transposed_forward_rounds_once_per_network(sg, name):
    """deconv_fwd_group2 on the stacked HALO3 launch: network A's images with A's fractional weights and bias, B's with B's, each
    y = store(act(exact)) of its own network -- the bias is added and the activation applied before the one rounding, per image."""
    from sggan_amd import _abi as A
    K = sg.kernels
    row = E.BY_NAME[name]
    pinned(row, "bf16")
    ea, eb = E.rounding(name, "bf16"), E.rounding(name, "bf16", "/B")
    g, xa, _, _, wda, ba = E.operands(sg, row, "bf16", ea)
    _, xb, _, _, wdb, bb = E.operands(sg, row, "bf16", eb)
    assert g.is_deconv and E.routes(g)[0] == "HALO3"
    yc = g.y_shape[3]
    pre = np.concatenate([padc(ea.y, yc), padc(eb.y, yc)])
    x = torch.cat([xa, xb])
    for act, leak, exp in ((A.ACT_NONE, 0.0, pre), (A.ACT_RELU, 0.0, np.maximum(pre, 0.0)), (A.ACT_LRELU, LEAK, E.lrelu_f32(pre, LEAK))):
        y = Guarded((2 * g.y_shape[0],) + tuple(g.y_shape[1:]), BF)
        K.deconv_fwd_group2(g, x, wda, ba, wdb, bb, act, leak, out=y.t)
        E.same(y.t, E.store(exp, BF), f"{name} group2 y act {act}")
        y.check(f"{name} group2 y act {act}")


# ---------------------------------------------------------------------------------------------------- c. fused forms, bf16
def nan_rows(shape):
    return Guarded(shape, F32, fill=float("nan"))


def sums_of_stored(part, ys, hw, what):
    """The statistics rows summed over their chunks (float64 on the host side): sum y_s EXACTLY the sum of the stored values, every
    partial sum a multiple of 1/128 below 2^24 of them; sum y_s^2 within 2 HW 2^-24 relative of the float64 sum of the stored squares
    -- HW non-negative terms, each exact in f32 (8 x 8 significant bits), summed in f32 in any order: at most HW - 1 additions, each
    within 2^-24 relative of a partial sum that never passes the total, a first-order bound of HW 2^-24, with a factor 2 over it."""
    assert not bool(torch.isnan(part.t).any()), f"{what}: a statistics row was not written"
    got = part.t.to(torch.float64).sum(1).cpu().numpy()
    exp = E.stat_sums(ys)
    E.same(got[..., 0], exp[..., 0], what + " sum y")
    rel = np.abs(got[..., 1] - exp[..., 1]) / np.maximum(exp[..., 1], 1e-300)
    print(f"{what}: sum y^2 max relative error {rel.max():.3e} (bound {2 * hw * 2.0 ** -24:.3e})")
    assert (exp[..., 1] > 0).any() and rel.max() <= 2 * hw * 2.0 ** -24, f"{what} sum y^2: relative error {rel.max():.3e}"
    part.check(what)


@pytest.mark.parametrize("name", E.STATS_FWD)
def test_forward_statistics_are_sums_of_the_stored_output(sg, name):
    K = sg.kernels
    row = E.BY_NAME[name]
    pinned(row, "bf16")
    e = E.rounding(name, "bf16")
    g, x, _, wf, _, b = E.operands(sg, row, "bf16", e)
    assert g.stats_chunks > 0
    yc = g.y_shape[3]
    y, part = Guarded(g.y_shape, BF), nan_rows((g.y_shape[0], g.stats_chunks, yc, 2))
    K.conv_fwd_stats(g, x, wf, b, out=y.t, out_partial=part.t)
    ys = E.store(padc(e.y, yc), BF)
    E.same(y.t, ys, f"{name} y")
    y.check(f"{name} y")
    sums_of_stored(part, ys, g.y_shape[1] * g.y_shape[2], f"{name} statistics")


@pytest.mark.parametrize("name,nsplit", E.DECONV_STATS, ids=[f"{n}-nsplit{k}" for n, k in E.DECONV_STATS])
def test_transposed_conv_statistics_are_sums_of_the_stored_output(sg, name, nsplit):
    K = sg.kernels
    row = E.BY_NAME[name]
    pinned(row, "bf16")
    ea = E.rounding(name, "bf16")
    tag = f"{name} nsplit {nsplit}"
    if nsplit:
        eb = E.rounding(name, "bf16", "/B")
        g = E.geom_n(row, "bf16", 2 if row[7] == 1 else row[7])
        xc, yc = g.x_shape[3], g.y_shape[3]
        _, wda = K.pack_weights(dev(ea.w), yc, xc, BF)
        _, wdb = K.pack_weights(dev(eb.w), yc, xc, BF)
        pair = (wdb, dev(padc(eb.b, yc)), nsplit)
        x, ye = dev(padc(E.round_paired(name, nsplit, "x"), xc), BF), padc(E.round_paired(name, nsplit, "y"), yc)
        ba = dev(padc(ea.b, yc))
        assert 0 < nsplit < g.x_shape[0]
    else:
        g, x, _, _, wda, ba = E.operands(sg, row, "bf16", ea)
        ye, pair = padc(ea.y, g.y_shape[3]), None
    assert g.is_deconv and g.stats_chunks == E.row_eligible(row, "bf16")[0] > 0 and E.routes(g)[0] == "S2HALO"
    y, part = Guarded(g.y_shape, BF), nan_rows((g.y_shape[0], g.stats_chunks, g.y_shape[3], 2))
    K.deconv_fwd_stats(g, x, wda, ba, pair, out=y.t, out_partial=part.t)
    ys = E.store(ye, BF)
    E.same(y.t, ys, tag + " y")
    y.check(tag + " y")
    sums_of_stored(part, ys, g.y_shape[1] * g.y_shape[2], tag + " statistics")


def test_norm_backward_sums_are_formed_from_the_stored_data_gradient(sg, bwd_name):
    """(sum g, sum g xhat), g = dx_s act'(z), with norm_bwd_case's operands: dx_s the STORED dx, a multiple of 1/128, act' in
    {0, 0.5, 1} and xhat an integer, every partial sum inside f32 (the CPU suite's bound) -- both sums exact."""
    from sggan_amd import _abi as A
    K = sg.kernels
    name = bwd_name
    row = E.BY_NAME[name]
    pinned(row, "bf16")
    e = E.rounding(name, "bf16")
    g, _, dy, _, wd, _ = E.operands(sg, row, "bf16", e)
    assert g.bwd_stats_chunks > 0
    c = E.norm_bwd_case(name)
    assert c.nx.shape == g.x_shape
    nx, st, gam, bet = dev(c.nx, BF), dev(c.stats), dev(c.gamma), dev(c.beta)
    add = E.frac_addend(name, e.x.shape, "bf16")
    pshape = (g.x_shape[0], g.bwd_stats_chunks, g.x_shape[3], 2)
    for addend in (None, add):
        dxs = E.store(e.dx + (0.0 if addend is None else addend), BF)
        for act, leak, an in ((A.ACT_NONE, 0.0, "none"), (A.ACT_RELU, 0.0, "relu"), (A.ACT_LRELU, 0.5, "lrelu")):
            tag = f"{name} addend={addend is not None} act={an}"
            dx, part = Guarded(g.x_shape, BF), nan_rows(pshape)
            K.conv_dgrad_stats(g, dy, wd, None if addend is None else dev(addend, BF), nx, st, gam, bet, act, leak, out=dx.t, out_partial=part.t)
            E.same(dx.t, dxs, tag + " dx")
            dx.check(tag + " dx")
            assert not bool(torch.isnan(part.t).any()), f"{tag}: a statistics row was not written"
            E.same(part.t.to(torch.float64).sum(1), E.norm_bwd_sums(dxs, c, an, leak), tag + " (sum g, sum g xhat)")
            part.check(tag + " partial")


def test_mixed_precision_data_gradient_is_not_rounded(sg, bwd_name):
    """bf16 operands, f32 result: dx (multiples of 1/128) plus nothing, a bf16 addend (k/8) or an f32 addend (odd integers around
    +-1001 plus k/4096) equals the oracle exactly -- neither the result nor the f32 addend passes through bf16."""
    K = sg.kernels
    name = bwd_name
    row = E.BY_NAME[name]
    pinned(row, "bf16")
    e = E.rounding(name, "bf16")
    g, _, dy, _, wd, _ = E.operands(sg, row, "bf16", e)
    assert g.dgrad_mixed
    for an, addend, adt in (("none", None, None), ("bf16", E.frac_addend(name, e.x.shape, "bf16"), BF), ("f32", E.frac_addend_f32(name, e.x.shape), F32)):
        dx = Guarded(g.x_shape, F32)
        out = K.conv_dgrad(g, dy, wd, None if addend is None else dev(addend, adt), out_f32=True, out=dx.t)
        assert out.data_ptr() == dx.t.data_ptr() and out.dtype == F32
        E.same(dx.t, e.dx + (0.0 if addend is None else addend), f"{name} f32 dx, addend {an}")
        dx.check(f"{name} f32 dx, addend {an}")


# ---------------------------------------------------------------------------------------------------- d. weight gradient, f32
@pytest.mark.parametrize("name", [n for n in WGRAD_ROWS if n not in WGRAD_LEFT_OUT])
def test_f32_weight_gradient_keeps_its_operands(sg, name):
    """x = k/2^f with f >= 9 fraction bits and integer dy: every product and every partial sum of dw is exact in f32 in any order
    and split, so dw equals the oracle exactly -- unless an operand loses mantissa on its way into the MFMA."""
    K = sg.kernels
    row = E.BY_NAME[name]
    pinned(row, "f32")
    c = E.wgrad_rounding(name)
    assert c.f >= WGRAD_MIN_F
    g = E.geom(row, "f32")
    x, dy = dev(padc(c.x, g.x_shape[3])), dev(padc(c.dy, g.y_shape[3]))
    tag = f"{name}[f32] {E.routes(g)[2]} f={c.f}"
    dw = Guarded(tuple(c.dw.shape), F32)
    (K.deconv_wgrad if g.is_deconv else K.conv_wgrad)(g, x, dy, dw.t)
    E.same(dw.t, c.dw, tag + " dw")
    dw.check(tag + " dw")
