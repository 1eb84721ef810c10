"""The convolution edge-case table shared by test_conv_edges_cpu.py (routes, eligibility, exactness bounds, sensitivity -- no GPU),
test_gpu_conv_edges.py (bit-exact parity of the plain calls on the device), test_gpu_conv_fused_edges.py (the same for the fused
and two-network forms) and test_gpu_conv_rounding.py (the one rounding of every epilogue: fractional draws, "rounding draws" below),
with the integer oracle, the exact comparison and the guard cells they share.

Every row is the smallest shape at which one route's index arithmetic can go wrong: a ragged last M tile, a channel tail
of one 8-channel granule, an odd parity class, the minimum a predicate admits and the first shape on either side of it.
Each row names the kernel every op runs on (sgg_conv2d_route / sgg_deconv2d_route, the code the launchers switch on), so
a threshold edit that moves a row to another kernel fails the CPU suite instead of silently un-testing the kernel.

Operands are drawn from {-1, 0, 1} (bias from [-2, 2]): every product and every partial sum in any order is an exact
integer, y and dx stay within bf16's exact-integer range (|v| <= 256) and dw / db below 2^24, so NO rounding rule enters
and any difference from the float64 oracle is an indexing bug.  The tolerance of test_gpu_ops.py (2e-2 of the tensor's
maximum in bf16) cannot see what stays below 2 % of the maximum: a whole missing input channel of the 1x1 row at Cin = 512
(1.6 %), one tap's share of a channel at Cin = 264 (a third of the 5.6 % the nine taps reach together), a handful of wrong
pixels; the exact comparison sees each (test_conv_edges_cpu.py::test_exact_comparison_sees_what_the_bf16_tolerance_misses).
"""
import functools
import zlib
from types import SimpleNamespace as NS

import numpy as np
import torch

from oracle import sggan_oracle as O

DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}

# (name, kind, R, stride, padding, Cin, Cout, N, H, W, {dtype: (forward, data-gradient, weight-gradient route, weight-gradient workspace)})
# The workspace is what sgg_conv2d_bwd_weight_workspace reports, in bytes: slab count x slab size, so it pins the planner's split
# count next to its route (recorded from the library before its launch layer was given one plan).
# deconv rows: H, W are the transposed conv's INPUT size.  Padding LEAD-1: zero padding with a LEADING pad of 1 and no trailing
# one -- a descriptor the library accepts and Keras 'SAME' never produces at an even size; run through kernels.py directly.
# The dtype set of a row is the key set of its route dict: the bf16-only kernel families run in bf16 alone (their f32 shapes
# take the generic routes other rows pin).  A comment above a row belongs to that row.
ROWS = [
    # generic GEMM tiles
    # Mmax 20806: last M tile 70 rows, second channel tile 8 columns, ktot_max 3; dgrad: 256x16 with the same ragged M
    ("glds_256x256_fwd_ragged", "conv", 3, 1, "SAME", 16, 264, 2, 101, 103, {"bf16": ("GLDS_256x256", "GLDS_256x16+SPLITK", "WGRAD_128x128", 12469248), "f32": ("GLDS_256x256", "GLDS_256x16+SPLITK", "WGRAD_128x128", 12469248)}),
    # the 256x256 tile on the data-gradient side
    ("glds_256x256_dgrad", "conv", 3, 1, "SAME", 264, 16, 2, 101, 103, {"bf16": ("GLDS_256x16+SPLITK", "GLDS_256x256", "WGRAD_128x16", 8211456), "f32": ("GLDS_256x16+SPLITK", "GLDS_256x256", "WGRAD_128x16", 8211456)}),
    # stride 2: four parity classes of unequal size (102x103, 102x102, 101x103, 101x102)
    ("glds_256x256_dgrad_s2", "conv", 3, 2, "SAME", 264, 16, 2, 203, 205, {"bf16": ("GLDS_256x16+SPLITK", "GLDS_256x256", "WGRAD_128x16", 8211456), "f32": ("GLDS_256x16+SPLITK", "GLDS_256x256", "WGRAD_128x16", 8211456)}),
    # M tail 109, channel tail 8, 324 blocks: not split
    ("glds_256x128_3stage", "conv", 3, 1, "SAME", 120, 392, 1, 79, 131, {"bf16": ("GLDS_256x128", "GLDS_128x64+SPLITK", "WGRAD_V2", 42336000), "f32": ("GLDS_256x128", "GLDS_128x64+SPLITK", "WGRAD_V2", 42336000)}),
    # 194 blocks: the in-kernel epilogue of a long reduction, not split
    ("glds_128x128_long_k", "conv", 3, 1, "SAME", 120, 136, 1, 100, 123, {"bf16": ("GLDS_128x128", "GLDS_128x64", "WGRAD_128x128", 28788480), "f32": ("GLDS_128x128", "GLDS_128x64", "WGRAD_128x128", 28788480)}),
    # forward split: DC 40, K-tiles 22 (bf16) / 43 (f32) over 5 / 10 splits
    ("splitk_fwd_dc40", "conv", 3, 1, "SAME", 152, 34, 1, 7, 9, {"bf16": ("GLDS_128x64+SPLITK", "GLDS_128x128", "WGRAD_128x64", 218880), "f32": ("GLDS_128x64+SPLITK", "GLDS_128x128", "WGRAD_128x64", 218880)}),
    # data gradient split: DC 40
    ("splitk_dgrad_dc40", "conv", 3, 1, "SAME", 34, 152, 1, 7, 9, {"bf16": ("GLDS_128x128", "GLDS_128x64+SPLITK", "WGRAD_128x128", 218880), "f32": ("GLDS_128x128", "GLDS_128x64+SPLITK", "WGRAD_128x128", 218880)}),
    # forward split: DC 264 (two full 128 tiles + 8), K-tiles 22 / 43 over 5 / 10
    ("splitk_fwd_dc264", "conv", 3, 1, "SAME", 152, 264, 2, 5, 13, {"bf16": ("GLDS_128x128+SPLITK", "GLDS_128x128+SPLITK", "WGRAD_V2", 2889216), "f32": ("GLDS_128x128+SPLITK", "GLDS_128x128+SPLITK", "WGRAD_V2", 2889216)}),
    # data gradient split: DC 264
    ("splitk_dgrad_dc264", "conv", 3, 1, "SAME", 264, 152, 2, 5, 13, {"bf16": ("GLDS_128x128+SPLITK", "GLDS_128x128+SPLITK", "WGRAD_128x128", 1444608), "f32": ("GLDS_128x128+SPLITK", "GLDS_128x128+SPLITK", "WGRAD_128x128", 1444608)}),
    # 1x1 window: one product per input channel (the sensitivity check's Cin >= 256 case); f32: 16 K-tiles over 4 splits
    ("pointwise_c512", "conv", 1, 1, "SAME", 512, 136, 1, 8, 9, {"bf16": ("GLDS_128x128", "GLDS_128x128", "WGRAD_128x128", 278528), "f32": ("GLDS_128x128+SPLITK", "GLDS_128x128", "WGRAD_128x128", 278528)}),
    # halo3: forward and data gradient, bf16
    ("halo3_min_reflect", "conv", 3, 1, "REFLECT-1", 64, 64, 1, 4, 128, {"bf16": ("HALO3", "HALO3", "WGRAD_128x64", 294912)}),   # H = 4: the fold's virtual rows dy[2]+dy[0] and dy[H-3]+dy[H-1] overlap
    ("halo3_min_same", "conv", 3, 1, "SAME", 64, 64, 1, 4, 128, {"bf16": ("HALO3", "HALO3", "WGRAD_128x64", 294912)}),
    # odd batch, two column tiles, destination tail of 8 in the second 256 tile
    ("halo3_n3_dtail_reflect", "conv", 3, 1, "REFLECT-1", 64, 264, 3, 6, 256, {"bf16": ("HALO3", "GLDS_128x64+SPLITK", "WGRAD_V2_ROWFAST", 21897216)}),
    ("halo3_n3_dtail_same", "conv", 3, 1, "SAME", 64, 264, 3, 6, 256, {"bf16": ("HALO3", "GLDS_128x64+SPLITK", "WGRAD_V2_ROWFAST", 21897216)}),
    # the destination tail on the data-gradient side (forward: 264 source channels, outside)
    ("halo3_dgrad_dtail_reflect", "conv", 3, 1, "REFLECT-1", 264, 64, 1, 4, 128, {"bf16": ("GLDS_128x64+SPLITK", "HALO3", "WGRAD_128x64", 1216512)}),
    ("halo3_dgrad_dtail_same", "conv", 3, 1, "SAME", 264, 64, 1, 4, 128, {"bf16": ("GLDS_128x64+SPLITK", "HALO3", "WGRAD_128x64", 1216512)}),
    # pair-eligible in BOTH directions (sgg_conv2d_pair_supported): odd batch, two column tiles, two 64-channel source chunks forward
    # (the halo refill), destination tail of 64 in the second 256 tile
    ("halo3_pair_n3_reflect", "conv", 3, 1, "REFLECT-1", 128, 320, 3, 4, 256, {"bf16": ("HALO3", "HALO3", "WGRAD_V2_ROWFAST", 35389440)}),
    ("halo3_pair_n3_same", "conv", 3, 1, "SAME", 128, 320, 3, 4, 256, {"bf16": ("HALO3", "HALO3", "WGRAD_V2_ROWFAST", 35389440)}),
    # the normalise-on-load table (H3_NORM_MAXC source channels) at its limit, and the first shape outside it: 576 source channels keep
    # the statistics epilogue (stats_chunks 4) and lose normload_ok
    ("halo3_normload_c512", "conv", 3, 1, "REFLECT-1", 512, 64, 2, 4, 128, {"bf16": ("HALO3", "HALO3", "WGRAD_128x64", 4718592)}),
    ("halo3_normload_out_c576", "conv", 3, 1, "REFLECT-1", 576, 64, 2, 4, 128, {"bf16": ("HALO3", "HALO3", "WGRAD_128x64", 5308416)}),
    ("halo3_out_h5", "conv", 3, 1, "REFLECT-1", 64, 64, 1, 5, 128, {"bf16": ("GLDS_128x64", "GLDS_128x64", "WGRAD_128x64", 442368)}),   # outside: odd H
    ("halo3_out_h2_reflect", "conv", 3, 1, "REFLECT-1", 64, 64, 1, 2, 128, {"bf16": ("GLDS_128x64", "GLDS_128x64", "WGRAD_128x64", 147456)}),   # outside: H = 2 < 4 (w9 admits it)
    ("halo3_out_h2_same", "conv", 3, 1, "SAME", 64, 64, 1, 2, 128, {"bf16": ("GLDS_128x64", "GLDS_128x64", "WGRAD_128x64", 147456)}),
    ("halo3_out_w120", "conv", 3, 1, "SAME", 64, 64, 1, 4, 120, {"bf16": ("GLDS_128x64", "GLDS_128x64", "WGRAD_128x64", 294912)}),   # outside: W one granule short of the tile
    ("halo3_out_w136", "conv", 3, 1, "REFLECT-1", 64, 64, 1, 4, 136, {"bf16": ("GLDS_128x64", "GLDS_128x64", "WGRAD_128x64", 442368)}),   # outside: W one granule past the tile
    ("halo3_out_c72", "conv", 3, 1, "REFLECT-1", 72, 72, 1, 4, 128, {"bf16": ("GLDS_128x64", "GLDS_128x64", "WGRAD_128x64", 373248)}),   # outside: 72 source channels in both directions
    # s2halo: stride-2 data gradient / transposed conv forward, bf16
    ("s2halo_min", "conv", 3, 2, "SAME", 64, 64, 1, 16, 64, {"bf16": ("GLDS_128x64", "S2HALO", "WGRAD_128x64", 147456)}),   # one 8 x 32 tile of dy
    ("s2halo_min_deconv", "deconv", 3, 2, "SAME", 64, 64, 1, 8, 32, {"bf16": ("S2HALO", "GLDS_128x64", "WGRAD_128x64", 147456)}),   # the same geometry as a transposed conv forward
    # 2 x 2 statistics tiles (16 x 64 output pixels each), two channel tiles, odd batch
    ("s2halo_deconv_n3", "deconv", 3, 2, "SAME", 128, 128, 3, 16, 64, {"bf16": ("S2HALO", "GLDS_128x128+SPLITK", "W9S", 28311552)}),
    # data gradient: 37 x 7 = 259 tiles on 130 persistent blocks, so two tiles per block and the last block owns one
    ("s2halo_tail_tile", "conv", 3, 2, "SAME", 448, 64, 37, 16, 64, {"bf16": ("GLDS_128x64+SPLITK", "S2HALO", "WGRAD_128x64", 33030144)}),
    ("s2halo_out_ho12", "conv", 3, 2, "SAME", 64, 64, 1, 24, 64, {"bf16": ("GLDS_128x64", "GLDS_128x64", "WGRAD_128x64", 294912)}),   # outside: Ho = 12
    ("s2halo_out_odd_h", "conv", 3, 2, "SAME", 64, 64, 1, 15, 64, {"bf16": ("GLDS_128x64", "GLDS_128x64", "WGRAD_128x64", 147456)}),   # outside: odd H (leading pad 1)
    ("s2halo_out_c72", "conv", 3, 2, "SAME", 72, 72, 1, 16, 64, {"bf16": ("GLDS_128x64", "GLDS_128x64", "WGRAD_128x64", 186624)}),   # outside: 72 channels
    # s2n: 3(8) -> 64 stride 2, data and weight gradient
    ("s2n_wo5", "conv", 3, 2, "SAME", 3, 64, 1, 6, 10, {"bf16": ("GLDS_128x64", "S2N", "S2N", 55296), "f32": ("GLDS_128x64", "GLDS_256x16", "WGRAD_128x64", 18432)}),   # Wo = 5: less than one 16-pixel item
    ("s2n_wo130", "conv", 3, 2, "SAME", 3, 64, 3, 4, 260, {"bf16": ("GLDS_128x64", "S2N", "S2N", 221184), "f32": ("GLDS_128x64", "GLDS_256x16", "WGRAD_128x64", 73728)}),   # Wo = 130: one 128-pixel segment plus 2
    # 7x7 head / stem, 5x5 narrow output
    ("head7_min", "conv", 7, 1, "REFLECT-3", 64, 3, 1, 8, 8, {"bf16": ("N7", "GLDS_128x64", "W7", 57344)}),   # the n7 minimum
    ("head7_ragged", "conv", 7, 1, "REFLECT-3", 64, 3, 2, 9, 65, {"bf16": ("N7", "GLDS_128x64", "W7", 458752)}),   # one row and one column past an 8 x 64 tile
    ("head7_16x32", "conv", 7, 1, "REFLECT-3", 64, 3, 1, 16, 32, {"bf16": ("N7", "HALO_NARROW_IN", "W7", 114688), "f32": ("HALO_FWD", "HALO_NARROW_IN", "HALO_WGRAD", 100352)}),
    ("head7_out_7x9", "conv", 7, 1, "REFLECT-3", 64, 3, 1, 7, 9, {"bf16": ("GLDS_256x16+SPLITK", "GLDS_128x64", "WGRAD_128x16", 100352)}),   # outside: H < 8
    # HALO_NARROW_IN forward, n7 data gradient
    ("stem7_16x32", "conv", 7, 1, "REFLECT-3", 3, 64, 1, 16, 32, {"bf16": ("HALO_NARROW_IN", "N7", "W7", 185600), "f32": ("HALO_NARROW_IN", "HALO_DGRAD_NARROW", "WGRAD_128x64", 200704)}),
    # 2 x 2 tiles of 16 x 32 pixels per image: the narrow-input kernel's statistics epilogue past one tile
    ("stem7_32x64_n2", "conv", 7, 1, "REFLECT-3", 3, 64, 2, 32, 64, {"bf16": ("HALO_NARROW_IN", "N7", "W7", 1232128)}),
    ("stem7_17x33", "conv", 7, 1, "REFLECT-3", 3, 64, 1, 17, 33, {"bf16": ("GLDS_128x64", "N7", "W7", 186624)}),   # generic forward, n7 data gradient
    ("stem7_min", "conv", 7, 1, "REFLECT-3", 3, 64, 2, 8, 8, {"bf16": ("GLDS_128x64", "N7", "W7", 235776)}),
    # narrow output: HALO_FWD, HALO_WGRAD
    ("narrow5_16x32", "conv", 5, 1, "SAME", 64, 8, 1, 16, 32, {"bf16": ("HALO_FWD", "HALO_NARROW_IN", "HALO_WGRAD", 51200), "f32": ("HALO_FWD", "HALO_NARROW_IN", "HALO_WGRAD", 51200)}),
    ("narrow5_17x32", "conv", 5, 1, "SAME", 64, 8, 1, 17, 32, {"bf16": ("GLDS_256x16+SPLITK", "GLDS_128x64", "WGRAD_128x16", 153600)}),   # the same one row taller: generic
    # narrow input: HALO_DGRAD_NARROW (the 64 -> 8 shape's data gradient is taken by HALO_NARROW_IN first)
    ("narrow5_in16_16x32", "conv", 5, 1, "SAME", 16, 64, 1, 16, 32, {"bf16": ("GLDS_128x64", "HALO_DGRAD_NARROW", "WGRAD_128x64", 204800), "f32": ("GLDS_128x64", "HALO_DGRAD_NARROW", "WGRAD_128x64", 204800)}),
    # REFLECT 2: the border fold's second launch behind HALO_DGRAD_NARROW, in its 64 x 16 tile (the only test of it in bf16); one 16 x 32
    # tile with p = 2 has two mirrored bands per side, the smallest shape whose band arithmetic differs from p = 1
    ("narrow5_in16_reflect", "conv", 5, 1, "REFLECT-2", 16, 64, 1, 16, 32,
     {"bf16": ("GLDS_128x64", "HALO_DGRAD_NARROW", "WGRAD_128x64", 204800),
      "f32":  ("GLDS_128x64", "HALO_DGRAD_NARROW", "WGRAD_128x64", 204800)}),
    ("narrow5_in16_17x32", "conv", 5, 1, "SAME", 16, 64, 1, 17, 32, {"bf16": ("GLDS_128x64", "GLDS_256x16+SPLITK", "WGRAD_128x64", 307200)}),   # one row taller: generic
    # weight gradients
    ("w9_min_reflect", "conv", 3, 1, "REFLECT-1", 64, 128, 1, 2, 64, {"bf16": ("GLDS_128x128", "GLDS_128x64+SPLITK", "W9", 294912)}),   # H = 2: row -1 mirrors to 1 and row 2 to 0
    ("w9_min_same", "conv", 3, 1, "SAME", 64, 128, 1, 2, 64, {"bf16": ("GLDS_128x128", "GLDS_128x64+SPLITK", "W9", 294912)}),
    # 2 tiles over 2 splits: the smallest shape at which the two-network launch gives each network a slab of its own
    ("w9_two_splits", "conv", 3, 1, "REFLECT-1", 64, 128, 1, 4, 64, {"bf16": ("GLDS_128x128", "GLDS_128x64+SPLITK", "W9", 589824)}),
    # 70 tiles over 35 splits; the odd split count has no two-network launch
    ("w9_odd_splits", "conv", 3, 1, "REFLECT-1", 64, 128, 5, 4, 448, {"bf16": ("GLDS_128x128", "GLDS_128x64+SPLITK", "W9", 10321920)}),
    ("w9_out_odd_h", "conv", 3, 1, "SAME", 64, 256, 2, 5, 64, {"bf16": ("GLDS_128x128", "GLDS_128x64+SPLITK", "WGRAD_V2_ROWFAST", 2949120)}),   # outside: odd H -> the row-fast DMA kernel with zero padding
    ("w9s_min", "conv", 3, 2, "SAME", 64, 128, 1, 2, 128, {"bf16": ("GLDS_128x128", "GLDS_128x64", "W9S", 294912)}),   # one output row: one split, so two networks take a launch each
    ("w9s_lead_pad", "conv", 3, 2, "LEAD-1", 64, 128, 1, 2, 128, {"bf16": ("GLDS_128x128", "GLDS_128x64", "W9S", 294912)}),   # pad_t = pad_l = 1 with H = 2 Ho: the halo's leading zero row / column
    ("w9s_two_splits", "conv", 3, 2, "SAME", 64, 128, 1, 4, 128, {"bf16": ("GLDS_128x128", "GLDS_128x64", "W9S", 589824)}),   # Ho 2: 2 tiles over 2 splits, two networks share the launch
    ("rowfast_valid", "conv", 3, 1, "VALID", 64, 256, 2, 6, 66, {"bf16": ("GLDS_128x128", "GLDS_128x64+SPLITK", "WGRAD_V2_ROWFAST", 2359296)}),   # Wo = 64 on VALID padding
    ("rowfast_7x7", "conv", 7, 1, "REFLECT-3", 8, 256, 1, 8, 64, {"bf16": ("GLDS_128x128", "GLDS_256x16+SPLITK", "WGRAD_V2_ROWFAST", 1605632)}),   # row-fast on a 7x7 window
    # f32 stages 32 pixels: row-fast at Wo = 32 (bf16: the gather form), odd H
    ("rowfast_f32_wo32", "conv", 3, 1, "SAME", 32, 256, 2, 5, 32, {"bf16": ("GLDS_128x128", "GLDS_128x64+SPLITK", "WGRAD_V2", 884736), "f32": ("GLDS_128x128", "GLDS_128x64+SPLITK", "WGRAD_V2_ROWFAST", 884736)}),
    ("wgrad_v2_wo63", "conv", 3, 1, "SAME", 64, 256, 1, 4, 63, {"bf16": ("GLDS_128x128", "GLDS_128x64+SPLITK", "WGRAD_V2", 1179648)}),   # gather form, one pixel short of a stage row
    ("wgrad_v2_wo65", "conv", 3, 1, "SAME", 64, 256, 1, 4, 65, {"bf16": ("GLDS_128x128", "GLDS_128x64+SPLITK", "WGRAD_V2", 1769472)}),   # gather form, one pixel past
    # Cr 3 of 8 stored, K tail 8
    ("wgrad_128x128_cr3", "conv", 3, 1, "SAME", 3, 136, 1, 9, 11, {"bf16": ("GLDS_128x128", "GLDS_256x16+SPLITK", "WGRAD_128x128", 39168), "f32": ("GLDS_128x128", "GLDS_256x16+SPLITK", "WGRAD_128x128", 39168)}),
    ("wgrad_128x64_cr3", "conv", 3, 2, "VALID", 3, 24, 1, 9, 11, {"bf16": ("GLDS_128x64", "GLDS_256x16", "WGRAD_128x64", 6912), "f32": ("GLDS_128x64", "GLDS_256x16", "WGRAD_128x64", 6912)}),   # Cr 3 of 8 stored
    ("wgrad_128x16_kr3", "conv", 3, 1, "SAME", 24, 3, 1, 9, 11, {"bf16": ("GLDS_256x16", "GLDS_128x64", "WGRAD_128x16", 6912), "f32": ("GLDS_256x16", "GLDS_128x64", "WGRAD_128x16", 6912)}),   # Kr 3 of 8 stored
    # transposed conv
    # outside s2halo: odd sizes, channel tails
    ("deconv_ragged", "deconv", 3, 2, "SAME", 24, 40, 2, 5, 7, {"bf16": ("GLDS_128x64", "GLDS_128x64", "WGRAD_128x64", 34560), "f32": ("GLDS_128x64", "GLDS_128x64", "WGRAD_128x64", 34560)}),
    # stride-1 transposed conv (the U-Net's d1-d8): the forward is the halo GEMM in its data-gradient direction WITH a bias and an
    # activation, the data gradient the forward GEMM, the weight gradient the conv's with x in the conv-output role
    ("tconv1_halo3_min", "deconv", 3, 1, "SAME", 64, 64, 1, 4, 128, {"bf16": ("HALO3", "HALO3", "WGRAD_128x64", 294912)}),
    # odd batch, two column tiles, destination tail of 8 forward
    ("tconv1_halo3_n3_dtail", "deconv", 3, 1, "SAME", 64, 264, 3, 6, 256, {"bf16": ("HALO3", "GLDS_128x64+SPLITK", "WGRAD_128x64", 10948608)}),
    # the tail on the data-gradient side
    ("tconv1_halo3_src264", "deconv", 3, 1, "SAME", 264, 64, 1, 4, 128, {"bf16": ("GLDS_128x64+SPLITK", "HALO3", "WGRAD_V2_ROWFAST", 2433024)}),
    # HALO3 both ways with Cin != Cout: two source chunks, destination tail of 64 in the second 256 tile
    ("tconv1_halo3_pair_n3", "deconv", 3, 1, "SAME", 128, 320, 3, 4, 256, {"bf16": ("HALO3", "HALO3", "W9", 35389440)}),
    # the U-Net's widest layer: eight source chunks
    ("tconv1_halo3_c512", "deconv", 3, 1, "SAME", 512, 512, 1, 4, 128, {"bf16": ("HALO3", "HALO3", "W9", 37748736)}),
    # d8: 3 (8) destination channels forward
    ("tconv1_head_c3", "deconv", 3, 1, "SAME", 64, 3, 3, 6, 256, {"bf16": ("HALO3", "GLDS_128x64", "WGRAD_128x64", 331776), "f32": ("GLDS_256x16+SPLITK", "GLDS_128x64", "WGRAD_128x64", 331776)}),
    # d8 off the halo kernel
    ("tconv1_head_ragged", "deconv", 3, 1, "SAME", 64, 3, 2, 9, 65, {"bf16": ("GLDS_256x16", "GLDS_128x64", "WGRAD_128x64", 92160), "f32": ("GLDS_256x16+SPLITK", "GLDS_128x64", "WGRAD_128x64", 92160)}),
    ("tconv1_out_h5", "deconv", 3, 1, "SAME", 64, 64, 1, 5, 128, {"bf16": ("GLDS_128x64", "GLDS_128x64", "WGRAD_128x64", 442368)}),   # outside: odd H
    ("tconv1_out_w120", "deconv", 3, 1, "SAME", 64, 64, 1, 4, 120, {"bf16": ("GLDS_128x64", "GLDS_128x64", "WGRAD_128x64", 294912)}),   # outside: W one granule short of the tile
    ("tconv1_out_c72", "deconv", 3, 1, "SAME", 72, 72, 1, 4, 128, {"bf16": ("GLDS_128x64", "GLDS_128x64", "WGRAD_128x64", 373248)}),   # outside: 72 source channels in both directions
    # split-K both ways with a bias behind the reduce
    ("tconv1_splitk", "deconv", 3, 1, "SAME", 152, 264, 2, 5, 13, {"bf16": ("GLDS_128x128+SPLITK", "GLDS_128x128+SPLITK", "WGRAD_128x128", 1444608), "f32": ("GLDS_128x128+SPLITK", "GLDS_128x128+SPLITK", "WGRAD_128x128", 1444608)}),
    ("tconv1_ragged", "deconv", 3, 1, "SAME", 24, 40, 2, 5, 7, {"bf16": ("GLDS_128x64", "GLDS_128x64", "WGRAD_128x64", 34560), "f32": ("GLDS_128x64", "GLDS_128x64", "WGRAD_128x64", 34560)}),
    # W9 with the operand roles swapped (x plays the conv-output side): one split with H = 2's mirrored rows; two slabs, so the grouped
    # call shares a launch; 35 slabs
    ("tconv1_w9_min", "deconv", 3, 1, "SAME", 128, 64, 1, 2, 64, {"bf16": ("GLDS_128x64+SPLITK", "GLDS_128x128", "W9", 294912)}),
    ("tconv1_w9_two_splits", "deconv", 3, 1, "SAME", 128, 64, 1, 4, 64, {"bf16": ("GLDS_128x64+SPLITK", "GLDS_128x128", "W9", 589824)}),
    ("tconv1_w9_odd_splits", "deconv", 3, 1, "SAME", 128, 64, 5, 4, 448, {"bf16": ("GLDS_128x64+SPLITK", "GLDS_128x128", "W9", 10321920)}),
]
# The routes of the U-Net generator's own layer shapes in bf16 (3x3, stride 1, SAME; conv e1-e8, transposed conv d1-d8; e5-e8 and d1-d4
# share one shape, 512 -> 512), at N8 128x128 and at N8 256x512 alike: a predicate narrowed for an edge row cannot move one unnoticed.
UNET_SIZES = [(8, 128, 128), (8, 256, 512)]
UNET_ROUTES = {
    "e1": ("conv", 3, 64, ("HALO_NARROW_IN", "HALO_DGRAD_NARROW", "WGRAD_128x64")), "e2": ("conv", 64, 128, ("HALO3", "HALO3", "W9")),
    "e3": ("conv", 128, 256, ("HALO3", "HALO3", "W9")), "e4": ("conv", 256, 512, ("HALO3", "HALO3", "W9")),
    "e5": ("conv", 512, 512, ("HALO3", "HALO3", "W9")), "d1": ("deconv", 512, 512, ("HALO3", "HALO3", "W9")),
    "d5": ("deconv", 512, 256, ("HALO3", "HALO3", "W9")), "d6": ("deconv", 256, 128, ("HALO3", "HALO3", "W9")),
    "d7": ("deconv", 128, 64, ("HALO3", "HALO3", "W9")), "d8": ("deconv", 64, 3, ("HALO3", "GLDS_128x64", "WGRAD_128x64")),
}
# The weight-gradient workspace of the bench workload's layers (tests/test_gpu_exact.LAYERS, bf16), recorded like the rows' from the
# library before its launch layer was given one plan: a planner edit cannot move a production layer's slab count unnoticed.
BENCH_WS_WGRAD = {
    "G.res_3x3_256": 75497472, "G.c2_s2_64_128": 75497472, "G.c3_s2_128_256": 60162048, "G.d1_T_256_128": 60162048, "G.d2_T_128_64": 75497472,
    "G.c1_7x7_3_64": 46273024, "G.out_7x7_64_3": 28901376, "D.h0_s2_3_64": 9437184, "D.h1_s2_64_128": 75497472, "D.h2_s2_128_256": 60162048,
    "D.h3_s1_256_512": 75497472, "D.h31_s2v_512": 66060288, "D.h32_s2v_512": 66060288, "D.h33_s1v_512": 47185920, "D.h4_s1_512_34": 2211840,
}
# The workspaces of the forward and the data gradient, {dtype: (ws_fwd, ws_dgrad)} in bytes as sgg_conv2d_fwd_workspace /
# sgg_conv2d_bwd_data_workspace (a transposed conv: the sgg_deconv2d_* queries) report them: the split-K slabs, a REFLECT data
# gradient's fold tensor in front of them, the padded grid of the N7 stem.  Recorded, for every row and dtype and for the bench layers
# in bf16, from the library before the forward and the data gradient were given one plan; rows and layers not listed need none: (0, 0).
WS_FWD_DGRAD = {
    "glds_256x256_fwd_ragged": {"bf16": (0, 2663168), "f32": (0, 2663168)}, "glds_256x256_dgrad": {"bf16": (2663168, 0), "f32": (2663168, 0)},
    "glds_256x256_dgrad_s2": {"bf16": (2689536, 0), "f32": (2689536, 0)}, "glds_256x128_3stage": {"bf16": (0, 9935040), "f32": (0, 9935040)},
    "splitk_fwd_dc40": {"bf16": (50400, 0), "f32": (100800, 0)}, "splitk_dgrad_dc40": {"bf16": (0, 50400), "f32": (0, 100800)},
    "splitk_fwd_dc264": {"bf16": (686400, 711360), "f32": (1372800, 1264640)}, "splitk_dgrad_dc264": {"bf16": (711360, 686400), "f32": (1264640, 1372800)},
    "pointwise_c512": {"f32": (156672, 0)}, "halo3_min_reflect": {"bf16": (0, 299520)}, "halo3_n3_dtail_reflect": {"bf16": (0, 16850432)},
    "halo3_n3_dtail_same": {"bf16": (0, 9437184)}, "halo3_dgrad_dtail_reflect": {"bf16": (1179648, 299520)},
    "halo3_dgrad_dtail_same": {"bf16": (1179648, 0)}, "halo3_pair_n3_reflect": {"bf16": (0, 8916480)},
    "halo3_normload_c512": {"bf16": (0, 599040)}, "halo3_normload_out_c576": {"bf16": (0, 599040)}, "halo3_out_h5": {"bf16": (0, 301824)},
    "halo3_out_h2_reflect": {"bf16": (0, 294912)}, "halo3_out_w136": {"bf16": (0, 317952)}, "halo3_out_c72": {"bf16": (0, 337152)},
    "s2halo_deconv_n3": {"bf16": (0, 6291456)}, "s2halo_tail_tile": {"bf16": (9699328, 0)}, "head7_min": {"bf16": (24576, 47104)},
    "head7_ragged": {"bf16": (449280, 639744)}, "head7_16x32": {"bf16": (196608, 197632), "f32": (262144, 395264)},
    "head7_out_7x9": {"bf16": (24192, 49408)}, "stem7_16x32": {"bf16": (0, 13376), "f32": (0, 3423232)}, "stem7_32x64_n2": {"bf16": (0, 85120)},
    "stem7_17x33": {"bf16": (0, 14352)}, "stem7_min": {"bf16": (0, 6272)}, "narrow5_16x32": {"bf16": (98304, 0), "f32": (196608, 0)},
    "narrow5_17x32": {"bf16": (104448, 0)}, "narrow5_in16_16x32": {"bf16": (0, 196608), "f32": (0, 393216)},
    "narrow5_in16_reflect": {"bf16": (0, 759808), "f32": (0, 1519616)}, "narrow5_in16_17x32": {"bf16": (0, 208896)},
    "w9_min_reflect": {"bf16": (0, 425984)}, "w9_min_same": {"bf16": (0, 131072)}, "w9_two_splits": {"bf16": (0, 566272)},
    "w9_odd_splits": {"bf16": (0, 19543040)}, "w9_out_odd_h": {"bf16": (0, 1474560)}, "rowfast_valid": {"bf16": (0, 1824768)},
    "rowfast_7x7": {"bf16": (0, 10196992)}, "rowfast_f32_wo32": {"bf16": (0, 368640), "f32": (0, 655360)}, "wgrad_v2_wo63": {"bf16": (0, 580608)},
    "wgrad_v2_wo65": {"bf16": (0, 599040)}, "wgrad_128x128_cr3": {"bf16": (0, 15840), "f32": (0, 28512)},
    # (a transposed conv's forward is the data-gradient GEMM: tconv1_splitk holds splitk_dgrad_dc264's two values the other way round)
    "tconv1_halo3_n3_dtail": {"bf16": (0, 9437184)}, "tconv1_halo3_src264": {"bf16": (1179648, 0)}, "tconv1_head_c3": {"f32": (589824, 0)},
    "tconv1_head_ragged": {"f32": (149760, 0)}, "tconv1_splitk": {"bf16": (686400, 711360), "f32": (1372800, 1264640)},
    "tconv1_w9_min": {"bf16": (131072, 0)}, "tconv1_w9_two_splits": {"bf16": (262144, 0)}, "tconv1_w9_odd_splits": {"bf16": (9175040, 0)},
    # the bench layers
    "G.res_3x3_256": {"bf16": (0, 14008320)}, "G.c1_7x7_3_64": {"bf16": (0, 17371648)}, "G.out_7x7_64_3": {"bf16": (0, 28675584)},
    "D.h31_s2v_512": {"bf16": (22855680, 0)}, "D.h32_s2v_512": {"bf16": (17203200, 15237120)}, "D.h33_s1v_512": {"bf16": (13844480, 17203200)},
    "D.h4_s1_512_34": {"bf16": (1331200, 0)},
}


def ws_fwd_dgrad(name, dtype):
    """The two workspaces the table records for a row or a bench layer."""
    return WS_FWD_DGRAD.get(name, {}).get(dtype, (0, 0))


# Rows whose dx passes bf16's exact-integer range: 49 taps x 256 output channels of +-1 products have a standard deviation of 75,
# so no draw keeps 4000 of them within 256.  The row is there for its weight gradient; its dx (at most 2^24: exact in f32 in any
# order) is compared after the ONE round-to-nearest-even to bf16 of store(), as test_gpu_exact.py compares the bench layers'.
DX_ROUNDS_ONCE = {"rowfast_7x7"}
# The host-only eligibility queries of a row in bf16 (ConvGeom: stats_chunks, bwd_stats_chunks, pair_ok, normload_ok, dgrad_mixed; a
# transposed conv's stats_chunks is sgg_deconv2d_fwd_stats_chunks), recorded from the library like the routes.  Rows not listed, and
# every row in f32, have no fused form: (0, 0, 0, 0, 0).  The first shape outside each predicate:
#   normload_ok: halo3_normload_out_c576 (C = 576 > H3_NORM_MAXC) keeps stats_chunks = 4 and loses normload_ok; the SAME rows have none
#   pair_ok:     halo3_min_* (N = 1); halo3_n3_dtail_* and halo3_dgrad_dtail_* (HALO3 in one direction only, the other splits K)
#   deconv stats_chunks: 0 in f32 (s2halo_min_deconv's f32 geometry, test_conv_edges_cpu.py) and outside s2halo_ok (deconv_ragged)
#   a stride-1 transposed conv (every tconv1_* row) has no statistics epilogue and no paired form, on HALO3 or off it: NO_FUSED
NO_FUSED = (0, 0, False, False, False)
ELIGIBLE = {
    "halo3_min_reflect": (4, 4, False, True, True), "halo3_min_same": (4, 4, False, False, True),
    "halo3_n3_dtail_reflect": (12, 0, False, True, False), "halo3_n3_dtail_same": (12, 0, False, False, False),
    "halo3_dgrad_dtail_reflect": (0, 4, False, False, True), "halo3_dgrad_dtail_same": (0, 4, False, False, True),
    "halo3_pair_n3_reflect": (8, 8, True, True, True), "halo3_pair_n3_same": (8, 8, True, False, True),
    "halo3_normload_c512": (4, 4, True, True, True), "halo3_normload_out_c576": (4, 4, True, False, True),
    "s2halo_min_deconv": (1, 0, False, False, False), "s2halo_deconv_n3": (4, 0, False, False, False),
    "stem7_16x32": (1, 0, False, False, False), "stem7_32x64_n2": (4, 0, False, False, False),
}
ROW_IDS = [r[0] for r in ROWS]
BY_NAME = {r[0]: r for r in ROWS}
CASES = [(r, dt) for r in ROWS for dt in r[10]]                         # one row's dtypes adjacent: its oracle is evaluated once
CASE_IDS = [f"{r[0]}-{dt}" for r, dt in CASES]


def parse_padding(padding):
    return ("VALID", int(padding.split("-")[1])) if padding.startswith("REFLECT") else (padding, 0)


def geom(row, dtype):
    """The ConvGeom ops.conv2d / ops.deconv2d resolve this row to (host only)."""
    from sggan_amd import kernels as K
    _, kind, R, stride, padding, Ci, Co, N, H, W, _ = row
    if kind == "deconv":
        return K.deconv_geom(N, H, W, K.cpad(Ci), K.cpad(Co), R, R, stride, DTYPES[dtype])
    if padding == "LEAD-1":
        from sggan_amd import _abi as A
        Ho, Wo = (H + 1 - R) // stride + 1, (W + 1 - R) // stride + 1
        d = A.ConvDesc(N, H, W, K.cpad(Ci), K.cpad(Co), R, R, stride, 1, 1, Ho, Wo, A.PAD_ZERO, K.dt(DTYPES[dtype]))
        return K.ConvGeom(d, (N, H, W, K.cpad(Ci)), (N, Ho, Wo, K.cpad(Co)), DTYPES[dtype], False)
    pad, refl = parse_padding(padding)
    return K.conv_geom(N, H, W, K.cpad(Ci), K.cpad(Co), R, R, stride, pad, refl, DTYPES[dtype])


def geom_n(row, dtype, n):
    """geom() of the row at another batch size: the stacked batch of the paired forms."""
    return geom(row[:7] + (n,) + row[8:], dtype)


def eligible(g):
    return (g.stats_chunks, g.bwd_stats_chunks, g.pair_ok, g.normload_ok, g.dgrad_mixed)


def row_eligible(row, dtype):
    """The eligibility the table names for a row."""
    return ELIGIBLE.get(row[0], NO_FUSED) if dtype == "bf16" else NO_FUSED


def routes(g):
    from sggan_amd import _abi as A
    return tuple(A.route_name(c) for c in (g.route_fwd, g.route_dgrad, g.route_wgrad))


def row_routes(row, dtype):
    """The three routes the table names for a row."""
    return row[10][dtype][:3]


def ints(rng, shape, lo=-1, hi=1):
    return rng.integers(lo, hi + 1, shape).astype(np.float64)


def inputs(row, net=""):
    """x, b, w of a row, seeded by its name; w in the Keras layout (conv HWIO, transposed conv (kh, kw, out, in))."""
    name, kind, R, _, _, Ci, Co, N, H, W, _ = row
    rng = np.random.default_rng(zlib.crc32((name + net).encode()))
    x = ints(rng, (N, H, W, Ci))
    b = ints(rng, (Co,), -2, 2)
    w = ints(rng, (R, R, Ci, Co) if kind == "conv" else (R, R, Co, Ci))
    return rng, x, b, w


def run_oracle(row, x, b, w, rng=None, dy=None):
    """Float64 oracle of the layer and its three gradients.  Per image where the im2col matrix would pass 0.5 GB (a convolution
    has no cross-image term; dw / db are sums over images, exact in integers).  dy: drawn from rng where not given."""
    _, kind, R, stride, padding, Ci, Co, N, H, W, _ = row
    lead = padding == "LEAD-1"                            # explicit zero pad of 1 on top and left only: a VALID conv of the padded input
    pad, refl = ("VALID", 0) if lead else parse_padding(padding)
    if lead:
        x = np.pad(x, ((0, 0), (1, 0), (1, 0), (0, 0)))
    ho, wo = (-(-H // stride), -(-W // stride)) if kind == "conv" else (H, W)
    chunk = N if N * ho * wo * R * R * Ci * 8 <= (1 << 29) else 1
    ys, dxs, dys, dw, db = [], [], [], 0.0, 0.0
    for n0 in range(0, N, chunk):
        t = O.Tape()
        vx, vb, vw = O.Var(x[n0:n0 + chunk]), O.Var(b), O.Var(w)
        yk = O.conv2d(t, vx, vw, vb, stride, pad, refl) if kind == "conv" else O.deconv2d(t, vx, vw, vb, stride)
        dyk = ints(rng, yk.v.shape) if dy is None else dy[n0:n0 + chunk]
        t.backward([(yk, dyk)])
        ys.append(yk.v); dxs.append(vx.g); dys.append(dyk)
        dw, db = dw + vw.g, db + vb.g
        del t, vx, yk
    dx = np.concatenate(dxs)
    return NS(y=np.concatenate(ys), dx=np.ascontiguousarray(dx[:, 1:, 1:]) if lead else dx, dw=dw, db=db, dy=np.concatenate(dys))


@functools.lru_cache(maxsize=2)
def expected(name):
    """Inputs and exact results of a row: evaluated once, shared by the tests of the row, never written to."""
    row = BY_NAME[name]
    rng, x, b, w = inputs(row)
    e = run_oracle(row, x, b, w, rng)
    e.x, e.b, e.w = x, b, w
    for a in vars(e).values():
        a.setflags(write=False)
    return e


# ---------------------------------------------------------------------------------------------------------------- rounding draws
# The draws of test_gpu_conv_rounding.py: the ONE rounding of every epilogue.  x and dy stay in {-1, 0, 1} (so REFLECT's pre-fold, which
# stores sums of up to four dy values in the operand type, stays exact); weights, bias and addend carry FRAC[dtype] fraction bits:
#   bf16: w = k/128 with |k| <= 128 (exact in bf16), bias = k/128 in [-2, 2], addend = k/8 in [-3, 3]
#   f32:  w = k/4096 with |k| <= 4096 (12-13 significant bits: more than bf16 or a 10-bit-mantissa operand path holds), bias and addend
#         likewise k/4096
# Every product is a multiple of 2^-f, so where sum |terms| 2^f < 2^24 per output element (bias and addend included) the f32
# accumulation is exact in ANY order and split, the float64 oracle is exact too, and the stored value is ONE round-to-nearest-even of
# it: store().  sum |terms| is the oracle run on |x|, |w|, |b|, |dy| (test_conv_edges_cpu.py asserts the bound for every case used).
FRAC = {"bf16": 7, "f32": 12}
# Two rows with 3 real channels on one side: 27 terms leave most sums below 2, where bf16 holds every multiple of 1/128, and the draw
# above misses a discrimination floor of test_conv_edges_cpu.py -- s2n_wo130: 23.7 % of y change under store (floor 25 %);
# wgrad_128x16_kr3: 21.8 % of dx (floor 25 %).  Their draw has no zeros in x and dy and no weight below 1/2: |w| < 1/2 is moved to
# |w| + 1/2.  (The other 3-channel rows keep the common draw: wgrad_128x128_cr3 25.1 % of y, wgrad_128x64_cr3 10.4 % from truncation.)
# The same on d8's shape as a transposed conv (3 real OUTPUT channels: 27 terms per element of dx) -- tconv1_head_c3: 21.0 % of dx,
# tconv1_head_ragged: 21.7 %.
ROUND_THIN = {"s2n_wo130", "wgrad_128x16_kr3", "tconv1_head_c3", "tconv1_head_ragged"}
# REFLECT rows whose bf16 data gradient is a narrow halo kernel on zero padding plus conv_border_fold_kernel, which rounds a second time
FOLD_TWICE = ["narrow5_in16_reflect", "head7_16x32"]


@functools.lru_cache(maxsize=3)
def rounding(name, dtype, net=""):
    """Inputs, exact results and sum |terms| (y_abs, dx_abs) of a row's rounding draw, seeded by name + "/round" (network B of the
    two-network forms: + "/B"): never written to, and evaluated once for the tests of a case that run next to each other
    (test_gpu_conv_rounding.py groups the tests of a case through a module-scoped parametrised fixture)."""
    row = BY_NAME[name]
    _, kind, R, _, _, Ci, Co, N, H, W, _ = row
    q = 2 ** FRAC[dtype]
    rng = seeded(name, "round" + net)
    x = ints(rng, (N, H, W, Ci))
    b = ints(rng, (Co,), -2 * q, 2 * q) / q
    w = ints(rng, (R, R, Ci, Co) if kind == "conv" else (R, R, Co, Ci), -q, q) / q
    e = run_oracle(row, x, b, w, rng)
    if name in ROUND_THIN:
        x = np.where(x == 0, 2 * ints(rng, x.shape, 0, 1) - 1, x)
        w = np.where(np.abs(w) < 0.5, np.where(w < 0, w - 0.5, w + 0.5), w)
        e = run_oracle(row, x, b, w, dy=np.where(e.dy == 0, 2 * ints(rng, e.dy.shape, 0, 1) - 1, e.dy))
    m = run_oracle(row, np.abs(x), np.abs(b), np.abs(w), dy=np.abs(e.dy))
    e.x, e.b, e.w, e.y_abs, e.dx_abs = x, b, w, m.y, m.dx
    del e.dw, e.db                                       # (not part of these cases: wgrad_rounding())
    for a in vars(e).values():
        a.setflags(write=False)
    e.f = FRAC[dtype]
    return e


def frac_addend(name, shape, dtype):
    """The fractional addend of a row's data gradient: k/8 in [-3, 3] in bf16 (exact there), k/4096 in [-3, 3] in f32."""
    q = 8 if dtype == "bf16" else 4096
    return ints(seeded(name, "round/addend"), shape, -3 * q, 3 * q) / q


def frac_addend_f32(name, shape):
    """The f32 addend of the mixed form: addend_f32's odd integers (bf16 holds none) plus k/4096 with |k| < 4096."""
    return addend_f32(name, shape) + ints(seeded(name, "round/addend_f32"), shape, -4095, 4095) / 4096


def truncate(a, dtype):
    """What an epilogue that TRUNCATES (drops the low mantissa bits of the f32 value) instead of rounding to nearest even stores."""
    t = torch.tensor(np.asarray(a, np.float64)).to(torch.float32)
    if dtype == torch.bfloat16:
        t = (t.view(torch.int32) & -65536).view(torch.float32)
    return t.to(torch.float64).numpy()


def lrelu_f32(v, leak):
    """The kernels' LeakyReLU on an exact f32 pre-activation: v > 0 ? v : float32(leak) * float32(v), one f32 rounding of the product."""
    v32 = np.asarray(v, np.float64).astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v)
    return np.where(v32 > 0, v32, np.float32(leak) * v32).astype(np.float64)


@functools.lru_cache(maxsize=2)
def fold_two_step(name):
    """The bf16 data gradient of a FOLD_TWICE row as the narrow halo routes compute it: the main launch pads with zeros and stores
    store(dx_zero); conv_border_fold_kernel reads that, adds the mirrored terms dx_reflect - dx_zero and rounds AGAIN.  Returns
    (band, value): band marks the elements where the REFLECT and the zero-padding oracle differ; off it the value is store(dx)."""
    row = BY_NAME[name]
    e = rounding(name, "bf16")
    assert row[1] == "conv" and row[3] == 1 and row[4].startswith("REFLECT")
    zero = run_oracle(row[:4] + ("SAME",) + row[5:], e.x, e.b, e.w, dy=e.dy)
    assert zero.y.shape == e.y.shape
    mirrored = e.dx - zero.dx
    band = mirrored != 0
    bf = torch.bfloat16
    two = np.where(band, store(store(zero.dx, bf) + mirrored, bf), store(e.dx, bf))
    band.setflags(write=False)
    two.setflags(write=False)
    return band, two


def round_paired(name, nsplit, field):
    """paired() of the rounding draws: images below nsplit from network A's tensor, the others from B's (an N = 1 row: A then B)."""
    a, b = getattr(rounding(name, "bf16"), field), getattr(rounding(name, "bf16", "/B"), field)
    return np.concatenate([a, b]) if a.shape[0] == 1 else np.concatenate([a[:nsplit], b[nsplit:]])


@functools.lru_cache(maxsize=2)
def wgrad_rounding(name):
    """The weight-gradient draw of an f32 row: x = k/2^f in [-1, 1], dy in {-1, 0, 1}, with the largest f <= 12 at which
    sum |x| |dy| 2^f < 2^24 holds for every element of dw (dw_abs: the oracle on |x|, |dy|), so dw is exact in f32 in any order and
    split.  k is drawn at 12 bits and truncated towards zero to f bits; `above` is sum |terms| of the draw at f + 1 bits, which
    missed the bound (None at f = 12)."""
    row = BY_NAME[name]
    _, kind, R, _, _, Ci, Co, N, H, W, _ = row
    rng = seeded(name, "round/wgrad")
    k = ints(rng, (N, H, W, Ci), -4096, 4096)
    w = np.zeros((R, R, Ci, Co) if kind == "conv" else (R, R, Co, Ci))
    b = np.zeros(Co)
    e = run_oracle(row, k / 4096, b, w, rng)
    dy, top, above = e.dy, None, None
    for f in range(12, 0, -1):
        x = np.trunc(k / 2 ** (12 - f)) / 2 ** f
        above, top = top, np.abs(run_oracle(row, np.abs(x), b, w, dy=np.abs(dy)).dw).max()
        if top * 2 ** f < 2 ** 24:
            break
    if f < 12:
        e = run_oracle(row, x, b, w, dy=dy)
    c = NS(x=x, dy=dy, dw=e.dw)
    for a in vars(c).values():
        a.setflags(write=False)
    c.f, c.dw_abs, c.above = f, top, above
    return c


def inputs_b(row):
    """An independent draw for "network B" of the two-network forms, seeded by name + "/B"."""
    return inputs(row, "/B")


@functools.lru_cache(maxsize=2)
def expected_b(name):
    """expected() of network B (x, w, b and dy of its own): a swapped weight, bias or batch offset changes values, not just order."""
    row = BY_NAME[name]
    rng, x, b, w = inputs_b(row)
    e = run_oracle(row, x, b, w, rng)
    e.x, e.b, e.w = x, b, w
    for a in vars(e).values():
        a.setflags(write=False)
    return e


def store(a, dtype):
    """What an exact real-valued result looks like after ONE round-to-nearest-even to the storage dtype."""
    return torch.tensor(np.asarray(a, np.float64)).to(torch.float32).to(dtype).to(torch.float64).numpy()


def mismatch(got, exp):
    """The exact comparison: None where got equals exp element for element, else a description of the first difference."""
    got = got.detach().to(torch.float64).cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    if got.shape != exp.shape:
        return f"shape {got.shape}, expected {exp.shape}"
    bad = got != exp
    if not bad.any():
        return None
    return f"{int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()} " \
           f"(got {got[bad][0]}, expected {exp[bad][0]}); max |diff| {np.abs(got - exp).max()}"


def same(got, exp, what):
    m = mismatch(got, exp)
    assert m is None, f"{what}: {m}"


# ---------------------------------------------------------------------------------------------------------------- fused forms
# The draws and float64 oracles of test_gpu_conv_fused_edges.py: the entry points a training step calls instead of the plain forward
# and data gradient.  test_conv_edges_cpu.py asserts the exactness bounds of every draw below on the oracle alone.
STATS_FWD = [r[0] for r in ROWS if r[1] == "conv" and ELIGIBLE.get(r[0], NO_FUSED)[0] > 0]        # conv_fwd_stats
STATS_BWD = [r[0] for r in ROWS if ELIGIBLE.get(r[0], NO_FUSED)[1] > 0]                           # conv_dgrad_stats, mixed precision
# (row, nsplit) of the paired forms; the N = 1 minimum rows are stacked A, B to N = 2
PAIRED = [("halo3_pair_n3_reflect", 1), ("halo3_pair_n3_reflect", 2), ("halo3_pair_n3_same", 1), ("halo3_pair_n3_same", 2),
          ("halo3_min_reflect", 1), ("halo3_min_same", 1)]
# (row, nsplit; 0: one network) of normalise on load
NORMLOAD = [("halo3_min_reflect", 0), ("halo3_pair_n3_reflect", 1), ("halo3_pair_n3_reflect", 2), ("halo3_normload_c512", 0)]
DECONV_STATS = [("s2halo_min_deconv", 0), ("s2halo_min_deconv", 1), ("s2halo_deconv_n3", 0), ("s2halo_deconv_n3", 1), ("s2halo_deconv_n3", 2)]
# Two-network grouped forward / data gradient / bias gradient, by the grp == 2 path the row reaches (asserted from its route):
# ragged last M tile; unequal stride-2 parity classes; split-K on each side (twice the single workspace); the stacked HALO3 rewrite
# (2N images, split at N); the REFLECT fold's two launches; stacked S2HALO (as data gradient and as transposed conv forward); stacked
# S2N; the special kernels' two launches; narrow5_in16_16x32, whose grouped data gradient an addend moves onto the generic GEMM;
# narrow5_in16_reflect, the same with the border fold's second launch behind each network's.
GROUP2 = ["glds_256x256_fwd_ragged", "glds_256x128_3stage", "glds_128x128_long_k", "glds_256x256_dgrad_s2",
          "splitk_fwd_dc40", "splitk_dgrad_dc40", "splitk_fwd_dc264", "splitk_dgrad_dc264", "pointwise_c512",
          "halo3_min_same", "halo3_n3_dtail_same", "halo3_n3_dtail_reflect", "halo3_dgrad_dtail_reflect",
          "s2halo_min", "s2halo_min_deconv", "s2halo_deconv_n3", "s2n_wo5", "s2n_wo130",
          "head7_ragged", "head7_16x32", "stem7_16x32", "stem7_17x33", "narrow5_16x32", "narrow5_in16_16x32", "narrow5_in16_reflect",
          "deconv_ragged", "wgrad_128x64_cr3",
          # stride-1 transposed convs: the stacked HALO3 launch in the data-gradient direction WITH a bias per image (forward) and in the
          # forward direction without one (data gradient), the generic GEMM's one launch on the other side of each, d8's 8 channels
          "tconv1_halo3_pair_n3", "tconv1_halo3_c512", "tconv1_halo3_n3_dtail", "tconv1_halo3_src264", "tconv1_head_c3", "tconv1_splitk",
          "tconv1_ragged"]
GROUP2_CASES = [(BY_NAME[n], dt) for n in GROUP2 for dt in BY_NAME[n][10]]
TWO_NETWORK = sorted({n for n, _ in PAIRED + DECONV_STATS} | set(GROUP2) | {"halo3_pair_n3_reflect"})


def seeded(name, what):
    return np.random.default_rng(zlib.crc32(f"{name}/{what}".encode()))


def addend(name, shape):
    """The integer addend of a row's data gradient (what test_gpu_conv_edges.py joins in the epilogue)."""
    return ints(np.random.default_rng(len(name)), shape, -3, 3)


def addend_f32(name, shape):
    """Odd integers around +-1001: exact in f32, not representable in bf16 (8 significant bits)."""
    rng = seeded(name, "addend_f32")
    return (1001.0 + 2 * ints(rng, shape, 0, 3)) * (2 * ints(rng, shape, 0, 1) - 1)


def paired(name, nsplit, field):
    """A stacked batch of two networks: images below nsplit from A's tensor, the others from B's (an N = 1 row: A then B)."""
    a, b = getattr(expected(name), field), getattr(expected_b(name), field)
    return np.concatenate([a, b]) if a.shape[0] == 1 else np.concatenate([a[:nsplit], b[nsplit:]])


def stat_sums(y):
    """(sum, sum of squares) per image and channel of a stored output: the statistics rows summed over their chunks."""
    return np.stack([y.sum((1, 2)), (y * y).sum((1, 2))], axis=-1)


def _pick(rng, values, shape):
    return np.asarray(values, np.float64)[rng.integers(0, len(values), shape)]


@functools.lru_cache(maxsize=2)
def norm_bwd_case(name):
    """The instance norm in front of a row's conv, for the norm-backward sums of its data gradient: every value from a set that
    keeps the kernel's f32 arithmetic exact.  mean in {-1, 0, 1} and rstd in {0.5, 1, 2} per (image, channel), gamma in
    {-2, -1, 1, 2}, beta an odd multiple of 0.5, x integers in [-2, 2] -- with x = mean wherever rstd = 0.5 and x - mean is odd, so
    that xhat = (x - mean) rstd is an integer everywhere; gamma xhat is then one too and z = gamma xhat + beta is never zero: the
    activation's derivative at z is unambiguous."""
    x = expected(name).x
    N, _, _, Cn = x.shape
    rng = seeded(name, "norm_bwd")
    mean, rstd = _pick(rng, (-1, 0, 1), (N, Cn)), _pick(rng, (0.5, 1, 2), (N, Cn))
    gamma, beta = _pick(rng, (-2, -1, 1, 2), (Cn,)), _pick(rng, (-1.5, -0.5, 0.5, 1.5), (Cn,))
    m4, r4 = mean[:, None, None, :], rstd[:, None, None, :]
    nx = ints(rng, x.shape, -2, 2)
    nx = np.where((r4 == 0.5) & ((nx - m4) % 2 != 0), m4, nx)
    xhat = (nx - m4) * r4
    c = NS(nx=nx, stats=np.stack([mean, rstd], axis=-1), gamma=gamma, beta=beta, xhat=xhat, z=gamma * xhat + beta)
    for a in vars(c).values():
        a.setflags(write=False)
    return c


def norm_bwd_sums(dx, c, act, leak=0.0):
    """(sum g, sum g xhat) per image and channel, g = dx act'(z): plain float64."""
    d = {"none": np.ones_like(c.z), "relu": (c.z > 0).astype(np.float64), "lrelu": np.where(c.z > 0, 1.0, leak)}[act]
    g = dx * d
    return np.stack([g.sum((1, 2)), (g * c.xhat).sum((1, 2))], axis=-1)


@functools.lru_cache(maxsize=2)
def normload_case(name):
    """Normalise on load: the raw operand, its (mean, rstd) and two networks' affine parameters, and what the kernel must make of
    them.  mean in {-1, 0, 1}, rstd in {0.5, 1, 2}, gamma in {-2, -1, 1, 2}, beta in {-1, 0}; x_raw = mean + t (2 t where rstd =
    0.5) with t in {-1, 0, 1}, two thirds of them zero, so xhat is an integer in [-2, 2] and x_norm = relu(gamma xhat + beta) one
    in [0, 4], one in eight non-zero (beta <= 0 keeps xhat = 0 at 0): the conv of it stays within bf16's exact integers up to 512
    source channels, where a denser draw (beta up to 1) reached |y| = 285.  Every product of
    the kernel's form x (gamma rstd) + (beta - mean gamma rstd) is a small dyadic number, exact in f32 fused or not.
    y[net]: the float64 conv of x_norm[net] with that network's weights and bias, all images."""
    row = BY_NAME[name]
    ea, eb = expected(name), expected_b(name)
    N, _, _, Cn = ea.x.shape
    rng = seeded(name, "normload")
    mean, rstd = _pick(rng, (-1, 0, 1), (N, Cn)), _pick(rng, (0.5, 1, 2), (N, Cn))
    m4, r4 = mean[:, None, None, :], rstd[:, None, None, :]
    t = ints(rng, ea.x.shape) * rng.integers(0, 2, ea.x.shape)
    x_raw = m4 + t * np.where(r4 == 0.5, 2.0, 1.0)
    xhat = (x_raw - m4) * r4
    c = NS(x_raw=x_raw, stats=np.stack([mean, rstd], axis=-1), gamma=[], beta=[], x_norm=[], y=[])
    for e in (ea, eb):
        gamma, beta = _pick(rng, (-2, -1, 1, 2), (Cn,)), _pick(rng, (-1, 0), (Cn,))
        xn = np.maximum(gamma * xhat + beta, 0.0)
        c.gamma.append(gamma); c.beta.append(beta); c.x_norm.append(xn)
        c.y.append(run_oracle(row, xn, e.b, e.w, dy=ea.dy).y)
    return c


def mix(a, b, nsplit):
    return np.concatenate([a[:nsplit], b[nsplit:]])


# ---------------------------------------------------------------------------------------------------------------- device side
def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a, np.float32)).to("cuda").to(dtype)


def padc(a, cp):
    """Zero channel padding to the stored channel count."""
    a = np.asarray(a)
    return a if a.shape[-1] == cp else np.concatenate([a, np.zeros(a.shape[:-1] + (cp - a.shape[-1],))], axis=-1)


def operands(sg, row, dtype, e, g=None):
    """The stored form of a row's tensors for the kernels.py launchers: channel-padded activations, packed weights, padded bias."""
    K = sg.kernels
    g = g or geom(row, dtype)
    dt = DTYPES[dtype]
    xc, yc = g.x_shape[3], g.y_shape[3]
    if g.is_deconv:                                      # w (kh, kw, out, in) is the HWIO kernel of the equivalent conv
        wf, wd = K.pack_weights(dev(e.w), yc, xc, dt)
    else:
        wf, wd = K.pack_weights(dev(e.w), xc, yc, dt)
    return g, dev(padc(e.x, xc), dt), dev(padc(e.dy, yc), dt), wf, wd, dev(padc(e.b, yc))


class Guarded:
    """A tensor inside a larger buffer filled with a sentinel: the bytes before and after it must survive the launch."""
    G = 4096

    def __init__(self, shape, dtype, fill=None):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.n = n
        self.buf = torch.full((2 * self.G + n,), 0xA5, dtype=torch.uint8, device="cuda")
        self.t = self.buf[self.G:self.G + n].view(dtype).view(shape)
        if fill is not None:
            self.t.fill_(fill)

    def check(self, what):
        assert bool((self.buf[:self.G] == 0xA5).all()), f"{what}: bytes before the tensor were written"
        assert bool((self.buf[self.G + self.n:] == 0xA5).all()), f"{what}: bytes after the tensor were written"

    def untouched(self, what):
        """Nothing at all was written: the tensor still holds the sentinel too."""
        assert bool((self.buf == 0xA5).all()), f"{what}: the output was written"
