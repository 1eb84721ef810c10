"""Throughput of the train step with the U-Net generator (generator_unet, module.py:125-206): bf16, HIP-graph replay, synthetic
inputs.  Prints one JSON line per size: images/s, ms/step, algorithmic TFLOP/s from the layer shapes, peak memory.

    python tools/bench_unet.py [--sizes 128x128x8,256x512x8] [--steps 10] [--warmup 3] [--cycle [--unpaired]] [--repeat R]

--cycle times the 2G+2D cycle step with two U-Nets (GeneratorUNetPair, both generators and both discriminators in lockstep);
--unpaired its one-network-at-a-time sequencing.  --repeat R runs every leg R times, interleaved (paired, unpaired, paired, ...
with --cycle --both), so that the legs of a comparison see the same machine state.

FLOPs: every U-Net layer is a 3x3 stride-1 'same' conv, 2*9*Cin*Cout FLOP per output pixel forward (43.9 MFLOP/px at ngf 64);
a reference-mode step is 3x the generator forward (forward, data gradient, weight gradient) + 7x the discriminator's, a cycle
step 12x + 14x, per image of ONE domain (bench.py's counts).
The per-layer kernel table comes from a separate `rocprofv3 --kernel-trace --stats` run of this script (profiles/unet_*)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

import sggan_amd
from bench import D_GMAC
from sggan_amd.module import unet_param_specs


def g_flop_per_px(ngf=64, in_c=3, out_c=3):
    return sum(2.0 * s[0] * s[1] * s[2] * s[3] for n, s in unet_param_specs(ngf, in_c, out_c) if n.endswith("_w"))


def d_flop_per_image(H, W):
    d = D_GMAC.get((H, W), 5.189 * (H * W) / (256 * 512))
    return 2e9 * d


def inputs(m, N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    real, seg = torch.rand((N, H, W, 3), generator=g), torch.rand((N, H, W, 3), generator=g)
    mh, mw = m.discriminator.out_hw(H, W)
    mh, mw = (round(H / 34), round(W / 34)) if (mh, mw) == (1, 1) else (mh, mw)
    idx = torch.randint(0, 34, (N, mh, mw), generator=g)
    return real, seg, torch.nn.functional.one_hot(idx, 34).float()


def run(N, H, W, steps, warmup, graph, cycle=False, paired=True):
    m = sggan_amd.sggan(sggan_amd.default_args(use_resnet=False, dtype="bf16", graph=graph, batch_size=N, image_height=H, image_width=W,
                                               cycle=cycle, paired=paired))
    m.real_A, m.seg_A, m.mask_A = inputs(m, N, H, W, 1)
    if cycle:
        m.real_B, m.seg_B, m.mask_B = inputs(m, N, H, W, 2)
    for _ in range(warmup):
        m.train_step()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.time()
    s.record()
    for _ in range(steps):
        m.train_step()
    e.record()
    torch.cuda.synchronize()
    ms = s.elapsed_time(e) / steps
    gl, dl = m.losses()
    gn, dn = (12, 14) if cycle else (3, 7)
    flop = N * (gn * g_flop_per_px() * H * W + dn * d_flop_per_image(H, W))
    work = ("cycle step, U-Net generators, " + ("paired" if paired else "one network at a time")) if cycle else "reference-mode step, U-Net generator"
    return {"workload": work, "dtype": "bf16", "graph": graph, "batch": N, "height": H, "width": W,
            "steps": steps, "warmup": warmup, "ms_per_step": round(ms, 3), "images_per_s": round(N * 1e3 / ms, 2),
            "tflop_per_step": round(flop / 1e12, 3), "tflops": round(flop / ms / 1e9, 1),
            "g_mflop_per_px_fwd": round(g_flop_per_px() / 1e6, 2), "wall_s": round(time.time() - t0, 2),
            "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 1e9, 2), "finite": bool(abs(gl) < float("inf") and abs(dl) < float("inf"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128x128x8,256x512x8", help="HxWxN,...")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eager", action="store_true", help="no HIP-graph replay")
    ap.add_argument("--cycle", action="store_true", help="the 2G+2D cycle step with two U-Nets")
    ap.add_argument("--unpaired", action="store_true", help="--cycle: one network at a time instead of the lockstep pairs")
    ap.add_argument("--both", action="store_true", help="--cycle: the paired and the unpaired leg, interleaved")
    ap.add_argument("--repeat", type=int, default=1, help="runs per leg")
    a = ap.parse_args()
    legs = [True, False] if (a.cycle and a.both) else [not a.unpaired]
    for sz in a.sizes.split(","):
        H, W, N = (int(v) for v in sz.split("x"))
        for rep in range(a.repeat):
            for paired in legs:
                print(json.dumps(dict(run(N, H, W, a.steps, a.warmup, not a.eager, a.cycle, paired), run=rep)), flush=True)
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()


if __name__ == "__main__":
    main()
