"""Host-side half of the convolution edge-case tests (no GPU): the route every row of tests/conv_edge_cases.py takes, the
exactness precondition of its integer oracle, and a proof that the exact comparison can fail where the tolerance of
test_gpu_ops.py cannot; the fused forms each row has (statistics epilogues, paired form, normalise on load, mixed precision) and the
exactness bounds of the draws test_gpu_conv_fused_edges.py runs them on; the exactness bound and the discrimination of the fractional
draws test_gpu_conv_rounding.py pins every epilogue's one rounding with."""
import ctypes

import numpy as np
import pytest
import torch

from sggan_amd import _abi as A
from tests import conv_edge_cases as E


@pytest.mark.parametrize("row", E.ROWS, ids=E.ROW_IDS)
def test_row_takes_the_route_the_table_names(row):
    for dtype in row[10]:
        assert E.routes(E.geom(row, dtype)) == E.row_routes(row, dtype), (row[0], dtype)


def test_every_route_is_pinned_by_a_row():
    named = [r for row in E.ROWS for dtype in row[10] for r in E.row_routes(row, dtype)]
    seen = {r.split("+")[0] for r in named}
    # REG: a reserved number that no query returns (the retired register-staged GEMM); it keeps the other routes' numbers in place
    assert seen == set(A.ROUTE_NAMES) - {"REG"}, set(A.ROUTE_NAMES) ^ seen
    split = {r for r in named if r.endswith("+SPLITK")}
    assert split and not any(r.startswith(("HALO", "S2", "N7", "W")) for r in split)     # only the generic GEMM tiles split K


# the slab count of the W9 rows that are there for it (a transposed conv's weight gradient is the conv's with x and dy swapped: the
# same tiles, the same splits)
W9_SPLITS = {"w9_two_splits": 2, "w9_odd_splits": 35, "tconv1_w9_min": 1, "tconv1_w9_two_splits": 2, "tconv1_w9_odd_splits": 35}


@pytest.mark.parametrize("row", E.ROWS, ids=E.ROW_IDS)
def test_row_keeps_its_weight_gradient_plan(row):
    """The planner's answer for the row -- the workspace the table records, i.e. its slab count -- and the precondition of the
    two-network test of test_gpu_conv_edges.py: operands (x, dy) and (2x, -dy) keep every partial sum of dw within
    2 N Ho Wo <= 2^24, exact in f32 in any summation order."""
    for dtype in row[10]:
        g = E.geom(row, dtype)
        assert g.ws_wgrad == row[10][dtype][3], (row[0], dtype)
        if E.row_routes(row, dtype)[2] == "W9":
            slab = 9 * g.desc.C * g.desc.K * 4                   # one f32 slab of dW per split: the workspace is the split count
            sp, tiles = g.ws_wgrad // slab, g.desc.N * (g.desc.H // 2) * (g.desc.W // 64)
            assert g.ws_wgrad == sp * slab and 1 <= sp <= tiles, (row[0], sp, tiles)
            if row[0] in W9_SPLITS:
                assert sp == W9_SPLITS[row[0]]
        assert 2 * g.desc.N * g.desc.Ho * g.desc.Wo <= 2 ** 24
    assert E.BY_NAME["w9s_two_splits"][10]["bf16"][3] == 2 * E.BY_NAME["w9s_min"][10]["bf16"][3]      # two slabs against one


def test_transposed_rows_that_share_a_grouped_weight_gradient_launch():
    """The slab count of each transposed row of the two-network weight-gradient test and whether its two networks run in one launch
    (W9: an even count; the LDS-DMA kernel: two slabs or more), from the workspace -- host only, so asserted here as well."""
    from tests import test_gpu_conv_edges as GE          # (module level: lists only, nothing touches a device)
    assert set(GE.TCONV1_SLABS) == {n for n in GE.GROUPED if n.startswith("tconv1_")}
    for name, exp in GE.TCONV1_SLABS.items():
        assert GE.shares_the_launch(E.geom(E.BY_NAME[name], "bf16")) == exp, name
    assert {s for s, _ in GE.TCONV1_SLABS.values()} >= {1, 2, 35}


def test_bench_layers_keep_their_weight_gradient_plan():
    """The same for the bench workload's layers (the shapes test_gpu_exact.py runs), against values recorded the same way."""
    from tests.test_gpu_exact import LAYERS
    assert set(E.BENCH_WS_WGRAD) == {l[0] for l in LAYERS}
    for l in LAYERS:
        g = E.geom(l + ({},), "bf16")
        assert g.ws_wgrad == E.BENCH_WS_WGRAD[l[0]], l[0]
        assert 2 * g.desc.N * g.desc.Ho * g.desc.Wo <= 2 ** 24


def test_rows_and_bench_layers_keep_their_forward_and_data_gradient_workspaces():
    """sgg_*_fwd_workspace / sgg_*_bwd_data_workspace for every row and dtype and every bench layer, against the recorded values:
    the split factor of the four split-K rows (_ktiles divides these), the fold tensor in front of the slabs, the N7 stem's grid."""
    from tests.test_gpu_exact import LAYERS
    names = {r[0] for r in E.ROWS} | {l[0] for l in LAYERS}
    assert set(E.WS_FWD_DGRAD) <= names, set(E.WS_FWD_DGRAD) - names
    for row, dtype in E.CASES:
        assert set(E.WS_FWD_DGRAD.get(row[0], {})) <= set(row[10]), row[0]
        g = E.geom(row, dtype)
        assert (g.ws_fwd, g.ws_dgrad) == E.ws_fwd_dgrad(row[0], dtype), (row[0], dtype)
    for l in LAYERS:
        g = E.geom(l + ({},), "bf16")
        assert (g.ws_fwd, g.ws_dgrad) == E.ws_fwd_dgrad(l[0], "bf16"), l[0]
    for row, dtype in E.CASES:                           # a split-K route has slabs
        for route, ws in zip(E.row_routes(row, dtype)[:2], E.ws_fwd_dgrad(row[0], dtype)):
            assert ws > 0 or not route.endswith("+SPLITK"), (row[0], dtype, route)


def test_route_query_rejects_bad_arguments():
    L = A.lib()
    ok = A.ConvDesc(1, 4, 128, 64, 64, 3, 3, 1, 1, 1, 4, 128, A.PAD_REFLECT, A.SGG_BF16)
    assert L.sgg_conv2d_route(ctypes.byref(ok), 0) == A.ROUTE["HALO3"]
    assert L.sgg_conv2d_route(ctypes.byref(ok), 3) == A.EINVAL and L.sgg_conv2d_route(ctypes.byref(ok), -1) == A.EINVAL
    assert L.sgg_deconv2d_route(ctypes.byref(ok), 0) == A.EINVAL                        # a transposed conv has no REFLECT form
    bad = A.ConvDesc(1, 8, 8, 7, 8, 3, 3, 1, 0, 0, 6, 6, 0, 0)                          # C not a multiple of 8
    assert L.sgg_conv2d_route(ctypes.byref(bad), 0) == A.EINVAL and L.sgg_deconv2d_route(ctypes.byref(bad), 2) == A.EINVAL
    assert L.sgg_conv2d_route(None, 0) == A.EINVAL


def test_bench_layers_keep_their_routes():
    """The routes of the bench workload's layers (test_gpu_exact.LAYERS): a predicate narrowed to move an edge shape to the
    generic kernel must not move one of these."""
    from tests.test_gpu_exact import LAYERS
    exp = {
        "G.res_3x3_256": ("HALO3", "HALO3", "W9"), "G.c2_s2_64_128": ("GLDS_128x128", "S2HALO", "W9S"),
        "G.c3_s2_128_256": ("GLDS_256x256", "S2HALO", "WGRAD_V2_ROWFAST"), "G.d1_T_256_128": ("S2HALO", "GLDS_256x256", "WGRAD_V2_ROWFAST"),
        "G.d2_T_128_64": ("S2HALO", "GLDS_128x128", "W9S"), "G.c1_7x7_3_64": ("HALO_NARROW_IN", "N7", "W7"),
        "G.out_7x7_64_3": ("N7", "HALO_NARROW_IN", "W7"), "D.h0_s2_3_64": ("GLDS_128x64", "S2N", "S2N"),
        "D.h1_s2_64_128": ("GLDS_128x128", "S2HALO", "W9S"), "D.h2_s2_128_256": ("GLDS_128x128", "S2HALO", "WGRAD_V2_ROWFAST"),
        "D.h3_s1_256_512": ("GLDS_256x128", "GLDS_128x128", "W9"), "D.h31_s2v_512": ("GLDS_128x128+SPLITK", "GLDS_128x128", "WGRAD_V2"),
        "D.h32_s2v_512": ("GLDS_128x128+SPLITK", "GLDS_128x128+SPLITK", "WGRAD_V2"),
        "D.h33_s1v_512": ("GLDS_128x128+SPLITK", "GLDS_128x128+SPLITK", "WGRAD_V2"), "D.h4_s1_512_34": ("GLDS_128x64+SPLITK", "GLDS_128x128", "WGRAD_128x64"),
    }
    assert set(exp) == {l[0] for l in LAYERS}
    for l in LAYERS:
        assert E.routes(E.geom(l + ({},), "bf16")) == exp[l[0]], l[0]


def test_unet_layers_keep_their_routes():
    """The same for the U-Net generator's own layers in bf16 (conv_edge_cases.UNET_ROUTES), at both sizes: e1 on the narrow-input
    kernels, e2-e8 and d1-d7 on HALO3 / HALO3 / W9, d8's forward on HALO3 with 8 destination channels.  No transposed layer has a
    fused form."""
    assert set(E.UNET_ROUTES) == {"e1", "e2", "e3", "e4", "e5", "d1", "d5", "d6", "d7", "d8"} and E.UNET_SIZES == [(8, 128, 128), (8, 256, 512)]
    for n, h, w in E.UNET_SIZES:
        for name, (kind, ci, co, exp) in E.UNET_ROUTES.items():
            g = E.geom((name, kind, 3, 1, "SAME", ci, co, n, h, w, {}), "bf16")
            assert E.routes(g) == exp, (name, n, h, w, E.routes(g))
            assert kind == "conv" or E.eligible(g) == E.NO_FUSED, (name, E.eligible(g))


def _ktiles(g, mode):
    """K-tile count and split factor of a zero-padded layer's forward (0) / data-gradient (1) GEMM: plan_conv's arithmetic, and
    its workspace (one f32 slab of the result per split, nothing else).  A transposed conv's forward is the data-gradient GEMM of its
    descriptor (the equivalent conv) and its data gradient the forward GEMM."""
    d, vec = g.desc, 8 if g.dtype == torch.bfloat16 else 4
    assert d.pad_mode == A.PAD_ZERO and d.stride == 1
    ws = g.ws_fwd if mode == 0 else g.ws_dgrad
    if (mode == 0) != g.is_deconv:
        return (d.R * d.S * (d.C // vec) + 7) // 8, ws // (d.N * d.Ho * d.Wo * d.K * 4), d.K
    return (d.R * d.S * (d.K // vec) + 7) // 8, ws // (d.N * d.H * d.W * d.C * 4), d.C


@pytest.mark.parametrize("name,mode", [("splitk_fwd_dc40", 0), ("splitk_dgrad_dc40", 1), ("splitk_fwd_dc264", 0), ("splitk_dgrad_dc264", 1),
                                       ("tconv1_splitk", 0), ("tconv1_splitk", 1)])
def test_split_k_rows_leave_a_remainder(name, mode):
    """The split-K rows' K-tile count is not divisible by the split factor, so the last split is shorter than the others."""
    row = E.BY_NAME[name]
    for dtype in row[10]:
        g = E.geom(row, dtype)
        assert E.row_routes(row, dtype)[mode].endswith("+SPLITK")
        ktot, ks, DC = _ktiles(g, mode)
        assert DC == ({0: 264, 1: 152}[mode] if name == "tconv1_splitk" else 40 if "dc40" in name else 264)
        assert ks >= 2 and ktot % ks != 0, (name, dtype, ktot, ks)


@pytest.mark.parametrize("row", E.ROWS, ids=E.ROW_IDS)
def test_row_is_exact_and_not_trivial(row):
    """The exactness precondition: y and dx within bf16's exact integers (|v| <= 256: one rounding to bf16 or f32 changes
    nothing), dw and db within f32's (< 2^24: exact in any summation order) -- and results large enough to mean something."""
    e = E.expected(row[0])
    assert np.abs(e.y).max() <= 256
    if row[0] in E.DX_ROUNDS_ONCE:
        assert 256 < np.abs(e.dx).max() < 2 ** 24        # (the exception is still one: see conv_edge_cases.DX_ROUNDS_ONCE)
    else:
        assert np.abs(e.dx).max() <= 256
    assert np.abs(e.dw).max() < 2 ** 24 and np.abs(e.db).max() < 2 ** 24
    assert np.abs(e.y).max() >= 8 and np.abs(e.dw).max() >= 8
    if row[0].startswith("tconv1_"):                     # (measured: |y| <= 206 and |dx| <= 197, both on tconv1_halo3_c512)
        assert np.abs(e.dw).max() >= 20
    for a in (e.y, e.dx, e.dw, e.db):
        assert np.array_equal(a, np.round(a))


def test_rows_whose_data_gradient_rounds_once():
    """The rows compared after one rounding of dx instead of as exact integers: rowfast_7x7 alone, no stride-1 transposed conv."""
    assert E.DX_ROUNDS_ONCE == {"rowfast_7x7"} and E.DX_ROUNDS_ONCE <= set(E.BY_NAME)
    assert sum(r[0].startswith("tconv1_") for r in E.ROWS) == 15


def _perturbed(row, e, how):
    """The oracle on an input with one thing missing -- what a kernel with that indexing bug would compute."""
    x, w = e.x.copy(), e.w.copy()
    if how == "channel":
        x[..., row[5] - 1] = 0                           # the last input channel: a K tail one channel short
    elif how == "tap":
        w[0, row[2] - 1] = 0                             # one tap of the window
    else:
        x[:, 0] = 0                                      # one border row of x
    return E.run_oracle(row, x, e.b, w, dy=e.dy)


@pytest.mark.parametrize("name", ["pointwise_c512", "splitk_dgrad_dc264", "halo3_dgrad_dtail_reflect"])
@pytest.mark.parametrize("how", ["channel", "tap", "border_row"])
def test_exact_comparison_sees_what_the_bf16_tolerance_misses(name, how):
    """Why this file exists.  A result computed with one input channel, one tap or one border row of x missing differs from
    the exact one, and the comparison test_gpu_conv_edges.py makes reports it in y (and in dx for the tap, in dw otherwise).
    The bf16 tolerance of test_gpu_ops.py (close(): 2e-2 of the tensor's maximum) does NOT report the missing channel of
    pointwise_c512 (Cin = 512): it changes y by at most 1 where max |y| is 61, 1.6 % of the maximum.  Measured for the
    record: on the two 3x3 rows (Cin = 264) the nine taps of the missing channel together reach 5.6 % of the maximum, which
    close() does report -- it is one tap's share of a channel (a third of that), a K tail short in one tap or a handful of
    wrong pixels that stay below its 2 %."""
    from tests.test_gpu_ops import close
    row = E.BY_NAME[name]
    e = E.expected(name)
    p = _perturbed(row, e, how)
    for dtype in row[10]:
        assert E.mismatch(E.store(p.y, E.DTYPES[dtype]), E.store(e.y, E.DTYPES[dtype])) is not None
        other = (p.dx, e.dx) if how == "tap" else (p.dw, e.dw)
        assert E.mismatch(*other) is not None
    if how == "channel" and name == "pointwise_c512":
        assert row[5] >= 256
        close(E.store(p.y, torch.bfloat16), E.store(e.y, torch.bfloat16), torch.bfloat16, "y with an input channel missing")   # passes


@pytest.mark.parametrize("how", ["channel", "tap", "other_bias"])
def test_exact_comparison_sees_a_transposed_conv_fault(how):
    """The same in the transposed direction, on tconv1_halo3_pair_n3 (128 -> 320, N3): the oracle with one input channel zeroed, with
    one tap zeroed, and with image 3 given network B's bias -- what a lockstep forward with a wrong per-image bias pick computes.
    The exact comparison reports each: in y, and in dw (channel) or dx (tap).  Measured against close() of test_gpu_ops.py (2e-2 of the
    tensor's maximum, max |y| = 111): at this width it reports all three as well -- the missing channel moves y by up to 9 (8.1 %),
    the tap by up to 36 (32 %), the bias by up to 4 (3.6 %) -- so what it cannot see here is the smaller share of each: one tap of one
    channel (at most 1), and the other network's bias wherever the two differ by 2 or less, 239 of the 320 channels of this draw
    (1.8 % of the maximum): a swap confined to those channels, or a pair of networks whose biases are that close, passes it."""
    from tests.test_gpu_ops import close
    name = "tconv1_halo3_pair_n3"
    row = E.BY_NAME[name]
    e, eb = E.expected(name), E.expected_b(name)
    bf = torch.bfloat16
    assert row[1] == "deconv" and row[7] == 3 and np.abs(e.y).max() == 111
    if how == "other_bias":
        y = e.y.copy()
        y[2] += eb.b - e.b
        step = np.abs(eb.b - e.b)
        assert step.max() == 4 and int((step / 111 < 2e-2).sum()) == 239 and int((step > 0).sum()) > 256
        assert not np.array_equal(y[2], e.y[2]) and np.array_equal(y[:2], e.y[:2])
    else:
        p = _perturbed(row, e, how)
        y = p.y
        assert E.mismatch(*((p.dx, e.dx) if how == "tap" else (p.dw, e.dw))) is not None
    assert E.mismatch(E.store(y, bf), E.store(e.y, bf)) is not None
    assert np.abs(y - e.y).max() == {"channel": 9, "tap": 36, "other_bias": 4}[how]
    with pytest.raises(AssertionError):                  # the tolerance reports it too, at the tensor's maximum
        close(E.store(y, bf), E.store(e.y, bf), bf, f"y with {how}")
    if how == "other_bias":                              # ... and not where the two biases differ by 2 or less
        small = step <= 2
        close(E.store(y, bf)[..., small], E.store(e.y, bf)[..., small], bf, "y with the other bias, close channels", scale=111.0)
        assert E.mismatch(E.store(y, bf)[..., small], E.store(e.y, bf)[..., small]) is not None


# ------------------------------------------------------------------------------------------------------------ fused forms
@pytest.mark.parametrize("row", E.ROWS, ids=E.ROW_IDS)
def test_row_keeps_its_fused_forms(row):
    """The host-only eligibility queries of the row -- statistics chunks forward and backward, the paired form, normalise on load,
    the mixed-precision data gradient -- against the table: a shape cannot lose or gain a fused form silently.  f32 has none."""
    for dtype in ("bf16", "f32"):
        g = E.geom(row, dtype)
        assert E.eligible(g) == E.row_eligible(row, dtype), (row[0], dtype, E.eligible(g))
        assert g.stats_chunks == 0 or E.routes(g)[0] in ("HALO3", "HALO_NARROW_IN", "S2HALO")
        assert g.bwd_stats_chunks == 0 or E.routes(g)[1] == "HALO3"


def test_first_shape_outside_each_fused_predicate():
    el = lambda name, dtype="bf16": E.eligible(E.geom(E.BY_NAME[name], dtype))           # noqa: E731
    # normalise on load: 512 source channels inside, 576 outside with the statistics epilogue kept; zero padding has no such form
    assert el("halo3_normload_c512")[3] and el("halo3_normload_c512")[0] > 0
    assert not el("halo3_normload_out_c576")[3] and el("halo3_normload_out_c576")[0] > 0
    assert not el("halo3_pair_n3_same")[3] and el("halo3_pair_n3_reflect")[3]
    # the paired form: not at N = 1 (the same shape at N = 2 has it), not where only one direction is HALO3
    for name in ("halo3_min_reflect", "halo3_min_same"):
        assert not el(name)[2] and E.geom_n(E.BY_NAME[name], "bf16", 2).pair_ok
    for name in ("halo3_n3_dtail_reflect", "halo3_n3_dtail_same", "halo3_dgrad_dtail_reflect", "halo3_dgrad_dtail_same"):
        r = E.row_routes(E.BY_NAME[name], "bf16")
        assert not el(name)[2] and E.BY_NAME[name][7] in (1, 3) and (r[0] == "HALO3") != (r[1] == "HALO3")
    assert not el("halo3_n3_dtail_same")[2] and E.BY_NAME["halo3_n3_dtail_same"][7] == 3            # (N >= 2: it is the routes)
    # transposed conv statistics: bf16 inside s2halo_ok only
    assert el("s2halo_min_deconv")[0] == 1 and el("s2halo_deconv_n3")[0] == 4
    assert el("s2halo_min_deconv", "f32")[0] == 0 and el("deconv_ragged")[0] == 0
    # ... and never at stride 1, on the halo kernel or off it, nor a paired form: the same shape as a conv has both
    for row in E.ROWS:
        if row[0].startswith("tconv1_"):
            assert row[1] == "deconv" and row[3] == 1 and E.row_eligible(row, "bf16") == E.NO_FUSED
            for dtype in ("bf16", "f32"):
                g = E.geom(row, dtype)
                assert g.stats_chunks == 0 and not g.pair_ok, (row[0], dtype)
    assert E.row_routes(E.BY_NAME["tconv1_halo3_pair_n3"], "bf16")[:2] == ("HALO3", "HALO3")
    assert el("halo3_pair_n3_same")[0] > 0 and el("halo3_pair_n3_same")[2]
    # the fused rows' lists hold what the issue names
    assert set(E.STATS_FWD) >= {"halo3_n3_dtail_reflect", "halo3_n3_dtail_same", "stem7_16x32", "stem7_32x64_n2"}
    assert set(E.STATS_BWD) >= {"halo3_dgrad_dtail_reflect", "halo3_dgrad_dtail_same"}
    assert E.geom(E.BY_NAME["halo3_dgrad_dtail_same"], "bf16").desc.C == 264


def _exact_ints(a, bound=256):
    return np.array_equal(a, np.round(a)) and np.abs(a).max() <= bound


@pytest.mark.parametrize("name", E.TWO_NETWORK)
def test_network_b_is_exact_and_unlike_network_a(name):
    """Network B's draw keeps the exactness bounds of the row's own, and differs from A in more than half the elements of every
    result: a two-network kernel that reads A's weights, bias or images for B cannot pass."""
    a, b = E.expected(name), E.expected_b(name)
    assert _exact_ints(b.y) and _exact_ints(b.dx)
    assert np.abs(b.dw).max() < 2 ** 24 and np.abs(b.db).max() < 2 ** 24 and np.abs(b.dy).sum((0, 1, 2)).max() < 2 ** 24
    for f in ("y", "dx", "dw", "x", "w", "dy"):
        assert (getattr(a, f) != getattr(b, f)).mean() > 0.5, (name, f)
    n2 = (2 * a.x.shape[0],) + a.x.shape[1:]
    add = E.addend(name, n2)                             # the grouped data gradient's addend over the stacked batch
    assert np.abs(np.concatenate([a.dx, b.dx]) + add).max() <= 256


@pytest.mark.parametrize("name", sorted(set(E.STATS_FWD) | {n for n, _ in E.PAIRED + E.DECONV_STATS}))
def test_statistics_sums_are_exact_in_f32(name):
    """(sum y, sum y^2) per image and channel of integers: below 2^24, so f32 holds every partial sum in any order."""
    for e in (E.expected(name), E.expected_b(name)):
        ys = E.store(e.y, torch.bfloat16)
        assert np.array_equal(ys, e.y) and E.stat_sums(ys).max() < 2 ** 24 and np.abs(ys).sum((1, 2)).max() < 2 ** 24


@pytest.mark.parametrize("name", E.STATS_BWD)
def test_norm_backward_draw_is_exact(name):
    e, c = E.expected(name), E.norm_bwd_case(name)
    mean, rstd = c.stats[..., 0], c.stats[..., 1]
    assert set(np.unique(mean)) <= {-1, 0, 1} and set(np.unique(rstd)) <= {0.5, 1, 2} and set(np.unique(c.gamma)) <= {-2, -1, 1, 2}
    assert np.array_equal(np.abs(c.beta) % 1, np.full(c.beta.shape, 0.5)) and _exact_ints(c.nx, 2) and _exact_ints(c.xhat, 6)
    assert np.abs(c.z).min() >= 0.5                      # never zero: the activation's derivative is unambiguous
    assert 0.2 < (c.z > 0).mean() < 0.8
    add = E.addend(name, e.x.shape)
    for dx in (e.dx, e.dx + add):
        assert _exact_ints(dx)                           # bf16 holds dx + addend
        # |g| <= |dx|, and the kernel's second sum is rstd (sum g x - mean sum g): every partial sum below 2^22 in units of 1/4
        assert (np.abs(dx) * (np.abs(c.nx) + 1)).sum((1, 2)).max() * 2 < 2 ** 22
        s = E.norm_bwd_sums(dx, c, "lrelu", 0.5)
        assert np.array_equal(s * 4, np.round(s * 4)) and np.abs(s).max() > 8
    # mixed precision: the f32 addend's odd integers pass bf16's range, the sum stays far inside f32's
    big = E.addend_f32(name, e.x.shape)
    assert np.abs(big).min() >= 1001 and np.all(big % 2 == 1) and np.abs(e.dx + big).max() < 2 ** 24
    assert (E.store(big, torch.bfloat16) != big).all()


@pytest.mark.parametrize("name,nsplit", E.PAIRED, ids=[f"{n}-nsplit{k}" for n, k in E.PAIRED])
def test_paired_draw_is_exact(name, nsplit):
    dx = E.paired(name, nsplit, "dx")
    assert _exact_ints(E.paired(name, nsplit, "y")) and _exact_ints(dx) and _exact_ints(dx + E.addend(name, dx.shape))
    n = 2 if E.BY_NAME[name][7] == 1 else E.BY_NAME[name][7]
    assert dx.shape[0] == n and 0 < nsplit < n


@pytest.mark.parametrize("name", sorted({n for n, _ in E.NORMLOAD}))
def test_normalise_on_load_draw_is_exact(name):
    c = E.normload_case(name)
    mean, rstd = c.stats[..., 0], c.stats[..., 1]
    assert set(np.unique(mean)) <= {-1, 0, 1} and set(np.unique(rstd)) <= {0.5, 1, 2} and _exact_ints(c.x_raw, 3)
    for k in (0, 1):
        assert set(np.unique(c.gamma[k])) <= {-2, -1, 1, 2} and _exact_ints(c.beta[k], 1)
        xn = c.x_norm[k]
        assert _exact_ints(xn) and xn.min() == 0 and 1 <= xn.max() <= 4 and (xn > 0).mean() > 0.1
        # the kernel's affine form x A + B with A = gamma rstd, B = beta - mean A: the same numbers, every term a small dyadic
        A_ = c.gamma[k] * rstd
        assert np.array_equal(np.maximum(c.x_raw * A_[:, None, None, :] + (c.beta[k] - mean * A_)[:, None, None, :], 0.0), xn)
        assert _exact_ints(c.y[k]) and np.abs(c.y[k]).max() >= 8 and E.stat_sums(c.y[k]).max() < 2 ** 24
    assert (c.x_norm[0] != c.x_norm[1]).mean() > 0.1 and (c.y[0] != c.y[1]).mean() > 0.5


def _chunk_sums(y, th, tw):
    """(sum, sumsq) rows of a th x tw pixel chunking: (N, chunks, C) each."""
    N, H, W, Cn = y.shape
    ch = y.reshape(N, H // th, th, W // tw, tw, Cn).transpose(0, 1, 3, 2, 4, 5).reshape(N, -1, th * tw, Cn)
    return ch.sum(2), (ch * ch).sum(2)


def test_exact_sums_see_a_dropped_statistics_row():
    """What the exact comparison of the statistics rows adds over the tolerances of test_conv_fwd_stats_epilogue
    (|d sum| < 1e-4 max + 1e-2, |d sumsq| < 1e-4 max), measured on a model of the chunking (a row per 128-pixel row segment of the
    3x3 kernel, per 16 x 64 output tile of the transposed conv, per 16 x 32 tile of the stem).
    - EVERY dropped row changes the exact (sum, sumsq) of its image and channel, on every row of the table.
    - In the sum, a dropped row can stay inside 1e-4 max + 1e-2: on s2halo_deconv_n3 (4 chunks, max |sum| above 10^4) there is a
      chunk whose sum is +-1.  This is the only such entry of the table's rows: the sums of squares, all terms positive, lose a
      share of about 1 / chunks with a dropped row, which the old relative tolerance does see on every row.  Measured for the
      record: what the tolerance could not see at these shapes is smaller than a row -- on s2halo_deconv_n3 one pixel in thirteen
      can be left out of its chunk inside both tolerances -- and the shapes themselves, which nothing ran."""
    tiles = {"halo3": (1, 128), "stem7": (16, 32), "s2halo": (16, 64)}
    inside_sum = {}
    for name in sorted(set(E.STATS_FWD) | {n for n, _ in E.DECONV_STATS}):
        ys = E.store(E.expected(name).y, torch.bfloat16)
        c1, c2 = _chunk_sums(ys, *tiles[name.split("_")[0]])
        assert c1.shape[1] == E.ELIGIBLE[name][0]
        assert (c2 > 0).all()                            # the exact sumsq changes with any dropped row
        s1, s2 = c1.sum(1), c2.sum(1)
        assert np.array_equal(np.stack([s1, s2], -1), E.stat_sums(ys))
        tol1, tol2 = 1e-4 * max(1.0, np.abs(s1).max()) + 1e-2, 1e-4 * s2.max()
        inside_sum[name] = int(((c1 != 0) & (np.abs(c1) < tol1)).sum())
        assert not (c2 < tol2).any()
        if name == "s2halo_deconv_n3":
            assert 0.05 < ((ys != 0) & (np.abs(ys) < tol1) & (ys * ys < tol2)).mean() < 0.10
    assert inside_sum["s2halo_deconv_n3"] >= 1 and sum(inside_sum.values()) == inside_sum["s2halo_deconv_n3"]


# ------------------------------------------------------------------------------------------------------------ rounding draws
# The draws of test_gpu_conv_rounding.py (conv_edge_cases.rounding), on the oracle alone: the exactness bound that makes store() of
# the float64 result THE expected value, and proof that each draw tells the faulty epilogues from the right one.
from tests import test_gpu_conv_rounding as RD          # noqa: E402  (module level: lists only, nothing touches a device)

BF = torch.bfloat16


def _share(a, b):
    return float((a != b).mean())


def _sig_bits(a, bits):
    """a rounded to `bits` significant bits (round to nearest): what an operand path with that mantissa makes of it."""
    m, ex = np.frexp(a)
    return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, ex)


def test_rounding_helpers():
    one = np.array([1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -7 + 2.0 ** -9, 0.0])
    assert np.array_equal(E.store(one, BF), [1, 1, 1 + 2.0 ** -6, -1, 1 + 2.0 ** -7, 0])           # ties to even
    assert np.array_equal(E.truncate(one, BF), [1, 1, 1 + 2.0 ** -7, -1, 1 + 2.0 ** -7, 0])        # towards zero
    assert np.array_equal(E.truncate(one, torch.float32), one)
    v = np.array([3.0, -3.0, -0.0078125, 0.0])
    assert np.array_equal(E.lrelu_f32(v, 0.5), [3, -1.5, -0.00390625, 0])
    l2 = E.lrelu_f32(v, 0.2)                                                                       # 0.2 is not exact in binary: one f32 product
    assert l2[1] == float(np.float32(0.2) * np.float32(-3.0)) and l2[1] != -3.0 * 0.2
    assert np.array_equal(_sig_bits(np.array([4095 / 4096, 0.5, 3 / 4096]), 11), [1.0, 0.5, 3 / 4096])


def _draws():
    """Every (row, dtype, network) draw test_gpu_conv_rounding.py evaluates: its forward / data-gradient cases, the bf16 draws of the
    statistics, norm-backward and mixed-precision rows, and network B of the two-network transposed-conv statistics."""
    d = [(r[0], dt, "") for r, dt in RD.CASES_AB]
    d += [(n, "bf16", "") for n in E.STATS_FWD + E.STATS_BWD + [n for n, _ in E.DECONV_STATS]]
    d += [(n, "bf16", "/B") for n, k in E.DECONV_STATS if k]
    d += [(n, "bf16", "/B") for n in RD.GROUPED_FWD]     # network B of the grouped transposed forward
    return list(dict.fromkeys(d))


_DRAWS = _draws()


@pytest.mark.parametrize("name,dtype,net", _DRAWS, ids=[f"{n}-{dt}{net.replace('/', '-')}" for n, dt, net in _DRAWS])
def test_rounding_draw_is_exact_and_discriminating(name, dtype, net):
    """Exactness: sum |terms| 2^f < 2^24 for y (bias included), dx and dx + addend, every value a multiple of 2^-f.
    Discrimination: at least 25 % of y and of dx change under store, at least 10 % differ from truncation and at least 10 % from
    adding the bias after the rounding.  In bf16 the store is the row's own; an f32 row stores its exact result unchanged
    (asserted), so there the floors are taken against bf16 -- the format a faulty path would pass through -- and a quarter of the
    weights does not survive an 11-significant-bit operand (a 10-bit mantissa)."""
    row = E.BY_NAME[name]
    e = E.rounding(name, dtype, net)
    q = 2.0 ** e.f
    assert e.f == E.FRAC[dtype] and set(np.unique(e.x)) <= {-1, 0, 1} and set(np.unique(e.dy)) <= {-1, 0, 1}
    for a in (e.w, e.b, e.y, e.dx):
        assert np.array_equal(a * q, np.round(a * q))
    assert np.abs(e.w).max() <= 1 and np.abs(e.b).max() <= 2
    assert np.array_equal(E.store(e.w, E.DTYPES[dtype]), e.w)
    assert (np.abs(e.y) <= e.y_abs).all() and (np.abs(e.dx) <= e.dx_abs).all()
    assert e.y_abs.max() * q < 2 ** 24 and e.dx_abs.max() * q < 2 ** 24
    if row[1] == "conv":
        add = E.frac_addend(name, e.x.shape, dtype)
        assert np.abs(add).max() <= 3 and np.array_equal(E.store(add, E.DTYPES[dtype]), add) and np.array_equal(add * q, np.round(add * q))
        assert (e.dx_abs + np.abs(add)).max() * q < 2 ** 24
        assert _share(E.store(e.dx + add, BF), e.dx + add) >= 0.25
    if dtype == "f32":
        assert np.array_equal(E.store(e.y, torch.float32), e.y) and np.array_equal(E.store(e.dx, torch.float32), e.dx)
        assert _share(_sig_bits(e.w, 11), e.w) >= 0.2
    ys = E.store(e.y, BF)
    shares = (_share(ys, e.y), _share(E.store(e.dx, BF), e.dx), _share(E.truncate(e.y, BF), ys),
              _share(E.store(E.store(e.y - e.b, BF) + e.b, BF), ys))
    print(f"{name}[{dtype}]{net}: bound y {e.y_abs.max() * q / 2 ** 24:.4f} dx {e.dx_abs.max() * q / 2 ** 24:.4f} of 2^24; "
          f"store changes y {shares[0]:.2f} dx {shares[1]:.2f}, truncation differs {shares[2]:.2f}, bias after rounding {shares[3]:.2f}")
    assert shares[0] >= 0.25 and shares[1] >= 0.25 and shares[2] >= 0.10 and shares[3] >= 0.10, shares
    # LeakyReLU 0.2 and its misplacement behind the rounding (bf16 rows; the f32 product is rounded once more on the way out)
    if dtype == "bf16":
        l = E.lrelu_f32(e.y, RD.LEAK)
        assert _share(E.store(E.lrelu_f32(ys, RD.LEAK), BF), E.store(l, BF)) >= 0.03


def test_reduced_operand_precision_changes_an_f32_row():
    """What the operand-precision check of the f32 rows sees: the same row with its weights at 11 significant bits (or at bf16's 8)
    differs from the exact result in nearly every element."""
    name = "splitk_fwd_dc40"
    e = E.rounding(name, "f32")
    for w in (_sig_bits(e.w, 11), E.store(e.w, BF)):
        p = E.run_oracle(E.BY_NAME[name], e.x, e.b, w, dy=e.dy)
        assert _share(p.y, e.y) > 0.9 and _share(p.dx, e.dx) > 0.9


_STAT_NETS = sorted({(n, "") for n in E.STATS_FWD} | {(n, "") for n, _ in E.DECONV_STATS} | {(n, "/B") for n, k in E.DECONV_STATS if k})


@pytest.mark.parametrize("name,net", _STAT_NETS, ids=[n + net.replace("/", "-") for n, net in _STAT_NETS])
def test_rounding_statistics_sums_are_exact_and_see_the_store(name, net):
    """sum y_s: stored values are multiples of 1/128, sum |y_s| 128 < 2^24 per (image, channel), so f32 holds every partial sum in any
    order.  The sum of the stored y differs from the sum of the exact y in at least 90 % of the pairs: rows summed from the accumulator
    cannot pass.  (sum y_s^2 is compared at a derived tolerance: test_gpu_conv_rounding.sums_of_stored.)"""
    e = E.rounding(name, "bf16", net)
    ys = E.store(e.y, BF)
    assert np.array_equal(ys * 128, np.round(ys * 128)) and np.abs(ys).sum((1, 2)).max() * 128 < 2 ** 24
    assert _share(ys.sum((1, 2)), e.y.sum((1, 2))) >= 0.9
    assert _share(E.stat_sums(ys)[..., 1], E.stat_sums(e.y)[..., 1]) >= 0.9
    if net:
        a = E.rounding(name, "bf16")
        for f in ("x", "w", "b", "y"):
            assert _share(getattr(a, f), getattr(e, f)) > 0.5, (name, f)


@pytest.mark.parametrize("name", E.STATS_BWD)
def test_rounding_norm_backward_and_mixed_draws_are_exact(name):
    e, c = E.rounding(name, "bf16"), E.norm_bwd_case(name)
    add = E.frac_addend(name, e.x.shape, "bf16")
    for dx in (e.dx, e.dx + add):
        dxs = E.store(dx, BF)
        assert _share(dxs, dx) >= 0.25
        # g = dx_s act'(z) is a multiple of 1/256 (act' = 0.5), x an integer; the kernel sums g and g x and forms rstd (sum g x - mean
        # sum g) with |mean| <= 1 and rstd a power of two: every partial sum is a multiple of 1/256 below 2^24 of them
        assert (np.abs(dxs) * (np.abs(c.nx) + 1)).sum((1, 2)).max() * 256 < 2 ** 24
        for act, leak in (("none", 0.0), ("relu", 0.0), ("lrelu", 0.5)):
            s, sx = E.norm_bwd_sums(dxs, c, act, leak), E.norm_bwd_sums(dx, c, act, leak)
            assert np.array_equal(s * 512, np.round(s * 512)) and np.array_equal(E.store(s, torch.float32), s)
            assert _share(s[..., 0], sx[..., 0]) >= 0.75           # sums formed from the unrounded dx differ (relu: some channels sum nothing)
    # mixed precision: dx in units of 1/128 plus an addend in units of 1/4096 around +-1001, exact in f32 and not in bf16
    big = E.frac_addend_f32(name, e.x.shape)
    assert np.abs(big).min() > 1000 and np.array_equal(big * 4096, np.round(big * 4096))
    assert (e.dx_abs + np.abs(big)).max() * 4096 < 2 ** 24
    for a in (e.dx, e.dx + add, e.dx + big):
        assert np.array_equal(E.store(a, torch.float32), a) and _share(E.store(a, BF), a) >= 0.25
    assert (E.store(big, BF) != big).all()


@pytest.mark.parametrize("name", E.FOLD_TWICE)
def test_border_fold_rounds_a_second_time_on_its_band(name):
    """The documented exception: in bf16 these REFLECT rows' data gradient is store(store(dx_zero) + mirrored terms) on the band the
    mirrored terms reach.  The two candidates differ there, so the device test tells them apart; off the band they are the same."""
    row = E.BY_NAME[name]
    assert E.row_routes(row, "bf16")[1] in ("HALO_NARROW_IN", "HALO_DGRAD_NARROW") and row[4].startswith("REFLECT")
    assert name in RD.ROWS_AB
    band, two = E.fold_two_step(name)
    one = E.store(E.rounding(name, "bf16").dx, BF)
    p = int(row[4].split("-")[1])
    inner = np.zeros(band.shape, bool)
    inner[:, 2 * p + 1:-(2 * p + 1), 2 * p + 1:-(2 * p + 1)] = True
    assert band.any() and not (band & inner).any()       # rows and columns 1..p and their mirror images only (0..2p bounds them)
    assert np.array_equal(two[~band], one[~band])
    print(f"{name}: {int((two != one).sum())} of {int(band.sum())} band elements differ between one and two roundings")
    assert (two != one)[band].any()


def test_weight_gradient_rounding_rows():
    """The f32 weight-gradient draw: the rows test_gpu_conv_rounding.py leaves out are exactly those whose bound holds fewer than 9
    fraction bits, at most half of the f32 rows."""
    assert RD.WGRAD_ROWS and all("f32" in E.BY_NAME[n][10] for n in RD.WGRAD_ROWS)
    assert 2 * len(RD.WGRAD_LEFT_OUT) <= len(RD.WGRAD_ROWS) and set(RD.WGRAD_LEFT_OUT) <= set(RD.WGRAD_ROWS)
    for name in RD.WGRAD_ROWS:
        c = E.wgrad_rounding(name)
        q = 2.0 ** c.f
        print(f"{name}: f = {c.f}, sum |terms| 2^f = {c.dw_abs * q / 2 ** 24:.3f} of 2^24")
        assert c.f <= 12 and c.dw_abs * q < 2 ** 24 and ((c.above is None) if c.f == 12 else c.above * 2 * q >= 2 ** 24)
        assert np.array_equal(c.x * q, np.round(c.x * q)) and np.abs(c.x).max() <= 1 and set(np.unique(c.dy)) <= {-1, 0, 1}
        assert np.array_equal(E.store(c.dw, torch.float32), c.dw) and np.abs(c.dw).max() <= c.dw_abs
        assert (c.f < RD.WGRAD_MIN_F) == (name in RD.WGRAD_LEFT_OUT), (name, c.f)
        if c.f >= RD.WGRAD_MIN_F:                         # x needs more bits than a bf16 operand holds (f = 12: than a 10-bit mantissa)
            assert _share(E.store(c.x, BF), c.x) >= 0.4 and _share(E.store(c.dw, BF), c.dw) >= 0.9
            assert c.f < 12 or _share(_sig_bits(c.x, 11), c.x) >= 0.2
