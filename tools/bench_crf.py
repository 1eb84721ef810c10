"""Cost of metric.dense_crf's device path (sgg_dense_crf, csrc/crf.hip) per image on one MI355X.

    python tools/bench_crf.py [--shapes 128x128x34,256x512x34] [--warmup 5] [--runs 20] [--out profiles/crf_bench.txt]

Each shape: a seeded blocky one-hot class mask and a noisy palette image (so the bilateral kernel is neither all ones nor all
zeros), `warmup` untimed calls, then `runs` calls each bracketed by its own pair of HIP events; the line reports the median,
minimum and maximum in ms, and beside them the two floors computed from the shape alone (N = H*W pixels, MAX_ITER = 10 steps
plus the normaliser pass):
  exp floor: 2 * N^2 * (MAX_ITER + 1) exponentials at 16 per clock per SIMD (v_exp_f32: a quarter of the 64-lane FMA rate)
  fma floor: 2 * N^2 * Cpad * MAX_ITER FMAs (two kernels, one FMA each per pair and channel) at 32 lanes per clock per SIMD
on 256 CUs x 4 SIMDs at 2.4 GHz.  Run the same command under `rocprofv3 --kernel-trace --stats` for the per-kernel split.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIMDS, CLOCK = 256 * 4, 2.4e9


def inputs(H, W, C, seed=0):
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, C, ((H + 7) // 8, (W + 7) // 8))
    labels = np.repeat(np.repeat(blocks, 8, axis=0), 8, axis=1)[:H, :W]
    palette = rng.integers(0, 256, (C, 3))
    img = np.clip(np.rint(palette[labels] + rng.normal(0.0, 2.0, (H, W, 3))), 0, 255).astype(np.uint8)
    probs = (np.arange(C)[:, None, None] == labels[None]).astype(np.float32)
    return torch.as_tensor(img).cuda(), torch.as_tensor(probs).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x128x34,256x512x34")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sggan_amd import kernels as K
    from sggan_amd import metric as M
    lines = []
    for shape in a.shapes.split(","):
        H, W, C = (int(v) for v in shape.split("x"))
        img, probs = inputs(H, W, C)
        ws = torch.empty(K.dense_crf_workspace_bytes(H, W, C), dtype=torch.uint8, device="cuda")
        out = torch.empty((C, H, W), dtype=torch.float32, device="cuda")
        run = lambda: K.dense_crf(img, probs=probs, max_iter=M.MAX_ITER, pos_w=M.POS_W, pos_xy_std=M.POS_XY_STD, bi_w=M.Bi_W,
                                  bi_xy_std=M.Bi_XY_STD, bi_rgb_std=M.Bi_RGB_STD, out=out, workspace=ws)
        for _ in range(a.warmup):
            run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        N = H * W
        exp_floor = 2.0 * N * N * (M.MAX_ITER + 1) / (16 * SIMDS * CLOCK) * 1e3
        fma_floor = 2.0 * N * N * K.cpad(C) * M.MAX_ITER / (32 * SIMDS * CLOCK) * 1e3
        lines.append(f"dense_crf {H}x{W}x{C}: median {statistics.median(ms):.3f} ms  min {min(ms):.3f}  max {max(ms):.3f}  "
                     f"({a.runs} runs after {a.warmup} warm-up; workspace {ws.numel() / 2 ** 20:.1f} MiB)  "
                     f"floors: exp {exp_floor:.3f} ms, fma {fma_floor:.3f} ms")
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
