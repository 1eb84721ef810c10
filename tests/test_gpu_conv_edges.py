"""Bit-exact parity of the convolution kernels at the route, tile and tail edges of tests/conv_edge_cases.py.

test_gpu_exact.py pins the kernels at the bench workload's shapes, where every extent is a multiple of every tile;
test_conv2d_fwd_bwd (test_gpu_ops.py) runs small and ragged shapes with a tolerance of 2e-2 of the tensor's maximum.  Here
the integer technique of the first runs at the smallest shapes where each route's index arithmetic can go wrong, and every
case asserts the route its shape takes (the CPU suite asserts the same: a threshold edit cannot move a row unnoticed).
Operands in {-1, 0, 1}: y and dx are exact integers within bf16's range, dw and db within f32's, so any difference from
the float64 oracle is an indexing bug, not a precision question."""
import numpy as np
import pytest
import torch

from tests import conv_edge_cases as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    import sggan_amd.kernels  # noqa: F401
    return sggan_amd


dev, padc, operands, Guarded = E.dev, E.padc, E.operands, E.Guarded     # (shared with test_gpu_conv_fused_edges.py)


@pytest.mark.parametrize("row,dtype", E.CASES, ids=E.CASE_IDS)
def test_edge_row_fwd_bwd_bit_exact(sg, row, dtype):
    name, kind, R, stride, padding = row[:5]
    dt = E.DTYPES[dtype]
    g = E.geom(row, dtype)
    assert E.routes(g) == E.row_routes(row, dtype)       # on this device's library too: a lab build or a config difference cannot hide a moved shape
    e = E.expected(name)
    tag = f"{name}[{dtype}] {E.row_routes(row, dtype)}"
    if padding == "LEAD-1":                              # no Keras padding gives this descriptor: the launchers of kernels.py directly
        K = sg.kernels
        g, x, dy, wf, wd, b = operands(sg, row, dtype, e)
        Cr, Kr = e.w.shape[2], e.w.shape[3]
        E.same(K.conv_fwd(g, x, wf, b), E.store(padc(e.y, g.y_shape[3]), dt), tag + " y")
        E.same(K.conv_dgrad(g, dy, wd), E.store(padc(e.dx, g.x_shape[3]), dt), tag + " dx")
        dw = torch.empty((R, R, Cr, Kr), dtype=torch.float32, device="cuda")
        K.conv_wgrad(g, x, dy, dw)
        E.same(dw, e.dw, tag + " dw")
        db = torch.empty(Kr, dtype=torch.float32, device="cuda")
        K.bias_grad(dy, db)
        E.same(db, e.db, tag + " db")
        return
    tx = dev(e.x, dt).requires_grad_(True)
    tw = dev(e.w).requires_grad_(True)
    tb = dev(e.b).requires_grad_(True)
    ty = sg.conv2d(tx, tw, tb, stride=stride, padding=padding) if kind == "conv" else sg.deconv2d(tx, tw, tb, stride=stride)
    E.same(ty, E.store(e.y, dt), tag + " y")
    ty.backward(dev(e.dy, dt))
    E.same(tx.grad, E.store(e.dx, dt), tag + " dx")
    E.same(tw.grad, e.dw, tag + " dw")
    E.same(tb.grad, e.db, tag + " db")


# Rows run through kernels.py for the fused forms of their routes -- forward + activation, data gradient + addend, weight
# gradient accumulated onto dw -- with every result inside sentinel guard cells: the ragged (or minimum) row of each family.
FUSED = ["glds_256x256_fwd_ragged", "glds_256x256_dgrad", "glds_256x128_3stage", "splitk_fwd_dc40", "splitk_dgrad_dc40",
         "splitk_fwd_dc264", "splitk_dgrad_dc264", "halo3_min_reflect", "halo3_n3_dtail_same", "halo3_dgrad_dtail_reflect",
         "s2halo_min", "s2halo_min_deconv", "s2n_wo130", "head7_ragged", "stem7_16x32", "stem7_17x33", "narrow5_16x32",
         "narrow5_in16_16x32", "w9_min_reflect", "w9_odd_splits", "w9s_min", "rowfast_valid", "rowfast_f32_wo32", "wgrad_v2_wo65",
         "wgrad_128x128_cr3", "wgrad_128x64_cr3", "wgrad_128x16_kr3", "deconv_ragged",
         "halo3_pair_n3_same", "s2halo_deconv_n3", "stem7_32x64_n2",     # two source chunks forward; S2HALO past one tile; the stem past one tile
         # stride-1 transposed convs: the halo GEMM's data-gradient direction with a bias and an activation (its epilogue off the plain
         # path, at 8 to 512 destination channels), the same behind a split-K reduce and on a ragged tile, W9 with x on the conv-output side
         "tconv1_halo3_min", "tconv1_halo3_n3_dtail", "tconv1_halo3_pair_n3", "tconv1_halo3_c512", "tconv1_head_c3", "tconv1_head_ragged",
         "tconv1_splitk", "tconv1_ragged", "tconv1_w9_two_splits"]
FUSED_CASES = [(E.BY_NAME[n], dt) for n in FUSED for dt in E.BY_NAME[n][10]]


@pytest.mark.parametrize("row,dtype", FUSED_CASES, ids=[f"{r[0]}-{dt}" for r, dt in FUSED_CASES])
def test_edge_row_fused_forms_in_guard_cells(sg, row, dtype):
    from sggan_amd import _abi as A
    K = sg.kernels
    name, R = row[0], row[2]
    dt = E.DTYPES[dtype]
    e = E.expected(name)
    g, x, dy, wf, wd, b = operands(sg, row, dtype, e)
    tag = f"{name}[{dtype}]"
    xc, yc = g.x_shape[3], g.y_shape[3]
    fwd = (lambda act, leak, out: K.deconv_fwd(g, x, wd, b, act, leak, out=out)) if g.is_deconv else \
          (lambda act, leak, out: K.conv_fwd(g, x, wf, b, act, leak, out=out))
    yp = padc(e.y, yc)
    for act, leak, f in ((A.ACT_NONE, 0.0, lambda v: v), (A.ACT_RELU, 0.0, lambda v: np.maximum(v, 0.0)),
                         (A.ACT_LRELU, 0.5, lambda v: np.where(v > 0, v, 0.5 * v))):     # halves of integers: exact in f32, one rounding to bf16
        y = Guarded(g.y_shape, dt)
        fwd(act, leak, y.t)
        E.same(y.t, E.store(f(yp), dt), f"{tag} y act {act}")
        y.check(f"{tag} y act {act}")
    # data gradient, plain and with an addend joined in the epilogue (conv only: the transposed conv has no such form)
    dxp = padc(e.dx, xc)
    dx = Guarded(g.x_shape, dt)
    if g.is_deconv:
        K.deconv_dgrad(g, dy, wf, out=dx.t)
    else:
        K.conv_dgrad(g, dy, wd, out=dx.t)
    E.same(dx.t, E.store(dxp, dt), tag + " dx")
    dx.check(tag + " dx")
    if not g.is_deconv:
        rng = np.random.default_rng(len(name))
        add = padc(E.ints(rng, e.x.shape, -3, 3), xc)    # (padding channels are zero in every stored tensor)
        dx = Guarded(g.x_shape, dt)
        K.conv_dgrad(g, dy, wd, dev(add, dt), out=dx.t)
        E.same(dx.t, E.store(dxp + add, dt), tag + " dx + addend")
        dx.check(tag + " dx + addend")
    # weight gradient written, then accumulated onto an integer-valued dw
    wshape = tuple(e.w.shape)
    for accumulate, base in ((False, 0.0), (True, 5.0)):
        dw = Guarded(wshape, torch.float32, fill=base if accumulate else None)
        (K.deconv_wgrad if g.is_deconv else K.conv_wgrad)(g, x, dy, dw.t, accumulate=accumulate)
        E.same(dw.t, e.dw + base, f"{tag} dw accumulate={accumulate}")
        dw.check(f"{tag} dw accumulate={accumulate}")


# Rows run through the two-network forms of the weight gradient (what the cycle step launches): every route of the family, the
# grouped call's shared launch (W9 / W9S from two splits on, the LDS-DMA kernel) and its launch per network (the others; W9 with an
# odd split count, W9S with one split).
GROUPED = ["narrow5_16x32", "head7_16x32", "head7_ragged", "stem7_17x33", "w9_min_reflect", "w9_odd_splits", "w9_two_splits", "w9s_min",
           "w9s_lead_pad", "w9s_two_splits", "s2n_wo130", "rowfast_valid", "rowfast_f32_wo32", "wgrad_v2_wo65", "wgrad_128x128_cr3",
           "wgrad_128x64_cr3", "wgrad_128x16_kr3", "deconv_ragged", "s2halo_deconv_n3",       # (W9S as a transposed conv)
           # stride-1 transposed convs (sgg_deconv2d_bwd_weight_group2: x on the conv-output side): W9 with one, two and 35 slabs and
           # with 24 at Cin != Cout, the LDS-DMA kernel, a generic tile
           "tconv1_w9_min", "tconv1_w9_two_splits", "tconv1_w9_odd_splits", "tconv1_halo3_pair_n3", "tconv1_halo3_src264", "tconv1_ragged"]
GROUPED_CASES = [(E.BY_NAME[n], dt) for n in GROUPED for dt in E.BY_NAME[n][10]]
# Which of the transposed rows' two networks share ONE launch, from the slab count (the workspace over one f32 slab of dW): W9 with
# an even count (half the slabs each), the LDS-DMA kernel from two slabs on; every other form launches once per network.
TCONV1_SLABS = {"tconv1_w9_min": (1, False), "tconv1_w9_two_splits": (2, True), "tconv1_w9_odd_splits": (35, False),
                "tconv1_halo3_pair_n3": (24, True), "tconv1_halo3_src264": (4, True), "tconv1_ragged": (1, False)}


def shares_the_launch(g):
    """(slab count, whether a grouped weight gradient of this shape runs both networks in one launch): run_wgrad's rule."""
    route = E.routes(g)[2]
    slabs, rest = divmod(g.ws_wgrad, 9 * g.desc.C * g.desc.K * 4)
    assert rest == 0
    return slabs, (route == "W9" and slabs % 2 == 0) or (route in ("WGRAD_V2", "WGRAD_V2_ROWFAST") and slabs >= 2)


@pytest.mark.parametrize("row,dtype", GROUPED_CASES, ids=[f"{r[0]}-{dt}" for r, dt in GROUPED_CASES])
def test_edge_row_two_network_weight_gradients_bit_exact(sg, row, dtype):
    """Network A is the row's (x, dy), network B (2x, -dy), stacked along the batch axis: dwA = dw and dwB = -2 dw, so a swapped
    operand pointer or swapped slabs change a sign or a factor.  Every operand is exact in bf16 and every partial sum stays
    within 2 N Ho Wo <= 2^24 (test_conv_edges_cpu.py asserts it), so the results are exact in ANY summation order -- the
    shared launches sum in another order than a single call -- and the row's one oracle run serves both networks."""
    K = sg.kernels
    name = row[0]
    e = E.expected(name)
    g, x, dy, _, _, _ = operands(sg, row, dtype, e)
    assert E.routes(g)[2] == E.row_routes(row, dtype)[2]
    tag = f"{name}[{dtype}] {E.row_routes(row, dtype)[2]}"
    if name in TCONV1_SLABS and dtype == "bf16":
        assert g.is_deconv and shares_the_launch(g) == TCONV1_SLABS[name], (name, shares_the_launch(g))
    xs, dys = torch.cat([x, 2 * x]), torch.cat([dy, -dy])
    wshape = tuple(e.w.shape)
    for accumulate in (False, True):
        dwa, dwb = Guarded(wshape, torch.float32, fill=5.0), Guarded(wshape, torch.float32, fill=-3.0)
        K.conv_wgrad_group2(g, xs, dys, dwa.t, dwb.t, accumulate=accumulate)
        E.same(dwa.t, e.dw + (5.0 if accumulate else 0.0), f"{tag} group2 dwA accumulate={accumulate}")
        E.same(dwb.t, -2 * e.dw + (-3.0 if accumulate else 0.0), f"{tag} group2 dwB accumulate={accumulate}")
        dwa.check(f"{tag} group2 dwA accumulate={accumulate}")
        dwb.check(f"{tag} group2 dwB accumulate={accumulate}")
    if E.row_routes(row, dtype)[2] != "W9" or g.is_deconv:   # (a transposed conv has no conv_wgrad_pair: g.wgrad_pair is False)
        assert not (g.is_deconv and g.wgrad_pair)
        return
    # two applications of one layer summed into one dw: dw(x, dy) + dw(2x, -dy) = -dw
    assert g.wgrad_pair
    for accumulate in (False, True):
        dwa = Guarded(wshape, torch.float32, fill=5.0)
        K.conv_wgrad_pair(g, x, dy, 2 * x, -dy, dwa.t, accumulate=accumulate)
        E.same(dwa.t, -e.dw + (5.0 if accumulate else 0.0), f"{tag} pair accumulate={accumulate}")
        dwa.check(f"{tag} pair accumulate={accumulate}")
    if name == "w9_two_splits":                          # ... of two networks: A as above, B dw(2x, dy) + dw(x, dy) = 3 dw
        for accumulate in (False, True):
            dwa, dwb = Guarded(wshape, torch.float32, fill=5.0), Guarded(wshape, torch.float32, fill=-3.0)
            assert K.conv_wgrad_pair2(g, (x, dy, 2 * x, -dy, dwa.t), (2 * x, dy, x, dy, dwb.t), accumulate=accumulate) is True
            E.same(dwa.t, -e.dw + (5.0 if accumulate else 0.0), f"{tag} pair2 dwA accumulate={accumulate}")
            E.same(dwb.t, 3 * e.dw + (-3.0 if accumulate else 0.0), f"{tag} pair2 dwB accumulate={accumulate}")
            dwa.check(f"{tag} pair2 dwA accumulate={accumulate}")
            dwb.check(f"{tag} pair2 dwB accumulate={accumulate}")


def test_odd_split_count_has_no_two_network_weight_gradient(sg):
    """w9_odd_splits: 70 pixel tiles over 35 splits.  The two-network launch gives each network half the splits, so an odd
    count has no such form: conv_wgrad_pair2 reports it and launches nothing."""
    K = sg.kernels
    row = E.BY_NAME["w9_odd_splits"]
    e = E.expected(row[0])
    g, x, dy, _, _, _ = operands(sg, row, "bf16", e)
    assert g.wgrad_pair and g.ws_wgrad // (9 * 64 * 128 * 4) == 35          # one f32 slab of dW per split
    dwa = torch.full(tuple(e.w.shape), 3.0, device="cuda")
    dwb = torch.full(tuple(e.w.shape), -7.0, device="cuda")
    assert K.conv_wgrad_pair2(g, (x, dy, x, dy, dwa), (x, dy, x, dy, dwb)) is False
    assert bool((dwa == 3.0).all()) and bool((dwb == -7.0).all())
    K.conv_wgrad_pair(g, x, dy, x, dy, dwa, accumulate=True)                  # the one-network pair form does exist
    E.same(dwa, 2 * e.dw + 3.0, "w9_odd_splits pair")
