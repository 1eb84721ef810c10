"""Host-side half of the convolution edge-case tests (no GPU): the route every row of tests/conv_edge_cases.py takes, the
exactness precondition of its integer oracle, and a proof that the exact comparison can fail where the tolerance of
test_gpu_ops.py cannot."""
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
    # REG: the register-staged GEMM, reachable only in a lab build with the DMA kernels switched off
    assert seen == set(A.ROUTE_NAMES) - {"REG"}, set(A.ROUTE_NAMES) ^ seen
    split = {r for r in named if r.endswith("+SPLITK")}
    assert split and not any(r.startswith(("HALO", "S2", "N7", "W")) for r in split)     # only the generic GEMM tiles split K


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
            if row[0] in ("w9_two_splits", "w9_odd_splits"):
                assert sp == (2 if row[0] == "w9_two_splits" else 35)
        assert 2 * g.desc.N * g.desc.Ho * g.desc.Wo <= 2 ** 24
    assert E.BY_NAME["w9s_two_splits"][10]["bf16"][3] == 2 * E.BY_NAME["w9s_min"][10]["bf16"][3]      # two slabs against one


def test_bench_layers_keep_their_weight_gradient_plan():
    """The same for the bench workload's layers (the shapes test_gpu_exact.py runs), against values recorded the same way."""
    from tests.test_gpu_exact import LAYERS
    assert set(E.BENCH_WS_WGRAD) == {l[0] for l in LAYERS}
    for l in LAYERS:
        g = E.geom(l + ({},), "bf16")
        assert g.ws_wgrad == E.BENCH_WS_WGRAD[l[0]], l[0]
        assert 2 * g.desc.N * g.desc.Ho * g.desc.Wo <= 2 ** 24


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


def _ktiles(g, mode):
    """K-tile count and split factor of a zero-padded conv's forward (0) / data-gradient (1) GEMM: plan_gemm's arithmetic, and
    its workspace (one f32 slab of the result per split, nothing else)."""
    d, vec = g.desc, 8 if g.dtype == torch.bfloat16 else 4
    assert not g.is_deconv and d.pad_mode == A.PAD_ZERO and d.stride == 1
    if mode == 0:
        return (d.R * d.S * (d.C // vec) + 7) // 8, g.ws_fwd // (d.N * d.Ho * d.Wo * d.K * 4)
    return (d.R * d.S * (d.K // vec) + 7) // 8, g.ws_dgrad // (d.N * d.H * d.W * d.C * 4)


@pytest.mark.parametrize("name,mode", [("splitk_fwd_dc40", 0), ("splitk_dgrad_dc40", 1), ("splitk_fwd_dc264", 0), ("splitk_dgrad_dc264", 1)])
def test_split_k_rows_leave_a_remainder(name, mode):
    """The split-K rows' K-tile count is not divisible by the split factor, so the last split is shorter than the others."""
    row = E.BY_NAME[name]
    for dtype in row[10]:
        g = E.geom(row, dtype)
        assert (g.desc.C if mode else g.desc.K) == (40 if "dc40" in name else 264)
        ktot, ks = _ktiles(g, mode)
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
    for a in (e.y, e.dx, e.dw, e.db):
        assert np.array_equal(a, np.round(a))


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
