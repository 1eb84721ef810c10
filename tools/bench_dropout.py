"""Cost of the U-Net decoder's training-mode dropout (csrc/dropout.hip) on one MI355X.

    python tools/bench_dropout.py [--warmup 3] [--runs 20] [--steps 10] [--repeats 2] [--no-step] [--out profiles/dropout_bench.txt]

Part 1, sgg_dropout alone, bf16, rate 0.5, at the shapes of a d1..d3 tensor of the U-Net step at 256x512 and at 128x128, batch 8 --
(8, 256*512*512) and (8, 128*128*512): `warmup` untimed calls, then `runs` calls each bracketed by its own pair of HIP events, once
"cold" -- a 512 MiB buffer is rewritten before every timed call, so nothing is left in the 256 MiB Infinity Cache -- and once
"warm" (calls back to back).  Median, minimum and maximum in us beside the byte floor (one 16-byte load and one 16-byte store per
vector) at the 6.29 TB/s a float4 copy reaches on this part.

Part 2, the U-Net reference step and the U-Net cycle step (one network at a time, the U-Net's default sequencing), bf16, 256x512,
batch 8, HIP-graph replay, built without and with dropout=0.5: per leg a fresh model, `warmup` steps, then `steps` replayed steps
between two HIP events; the legs take turns (`repeats` rounds of without, with) so that both see the same machine state, one model
resident at a time (a 256x512 cycle model holds tens of GB of activations).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.29e12          # bytes/s, measured float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--no-step", action="store_true", help="part 1 only")
    ap.add_argument("--no-cycle", action="store_true", help="part 2: the reference step only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_bench.txt"), help="where the lines are written ('' : nowhere)")
    a = ap.parse_args()
    import torch
    import sggan_amd
    from sggan_amd import kernels as K
    assert torch.cuda.is_available(), "bench_dropout.py measures on the GPU"
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    it = torch.zeros(1, dtype=torch.int64, device="cuda")
    for n, elems, what in ((8, 256 * 512 * 512, "256x512x512"), (8, 128 * 128 * 512, "128x128x512")):
        x = torch.rand((n, elems), device="cuda").to(torch.bfloat16)
        nbytes = 2.0 * x.numel() * 2
        for mode in ("cold", "warm"):
            for _ in range(a.warmup):
                K.dropout_(x, 0.5, it, 19, 0, 0)
            torch.cuda.synchronize()
            us = []
            for _ in range(a.runs):
                x.fill_(1.0)                      # (in place at scale 2: keep the values finite over the runs)
                if mode == "cold":
                    flush.fill_(1)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                K.dropout_(x, 0.5, it, 19, 0, 0)
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            med = statistics.median(us)
            say(f"dropout bf16 8x{what} {mode:4s}: median {med:7.1f} us  min {min(us):7.1f}  max {max(us):7.1f}  {nbytes / 1e6:7.1f} MB  "
                f"byte floor {nbytes / HBM * 1e6:6.1f} us  median / floor {med / (nbytes / HBM * 1e6):.2f}  {nbytes / med / 1e6:.2f} TB/s  "
                f"({a.runs} runs after {a.warmup} warm-up)")
        del x
    del flush
    torch.cuda.empty_cache()

    if not a.no_step:
        from tools.bench_unet import inputs
        N, H, W = 8, 256, 512
        for cycle in ((False,) if a.no_cycle else (False, True)):
            name = "U-Net cycle step (one network at a time)" if cycle else "U-Net reference step"
            ms = {"without": [], "with dropout": []}
            for rep in range(a.repeats):
                for tag, extra in (("without", {}), ("with dropout", {"dropout": 0.5})):
                    mdl = sggan_amd.sggan(sggan_amd.default_args(use_resnet=False, dtype="bf16", image_height=H, image_width=W, batch_size=N,
                                                                 cycle=cycle, graph=True, **extra))
                    mdl.real_A, mdl.seg_A, mdl.mask_A = inputs(mdl, N, H, W, 1)
                    if cycle:
                        mdl.real_B, mdl.seg_B, mdl.mask_B = inputs(mdl, N, H, W, 2)
                    for _ in range(a.warmup):
                        mdl.train_step()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.steps):
                        mdl.train_step()
                    e1.record()
                    e1.synchronize()
                    ms[tag].append(e0.elapsed_time(e1) / a.steps)
                    gl, dl = mdl.losses()
                    assert abs(gl) < float("inf") and abs(dl) < float("inf")
                    del mdl
                    torch.cuda.empty_cache()
            for tag, xs in ms.items():
                say(f"{name} bf16 {H}x{W} batch {N}, graph replay, {tag:12s}: ms/step per leg of {a.steps} " + " ".join(f"{v:.3f}" for v in xs) +
                    f"  median {statistics.median(xs):.3f}")
            m0, m1 = statistics.median(ms["without"]), statistics.median(ms["with dropout"])
            apps = 4 if cycle else 1
            say(f"{name}: with dropout / without = {m1 / m0:.4f} ({m1 - m0:+.3f} ms per step: {apps} generator application(s), each 3 masks forward, "
                f"3 backward and 3 bias gradients over 8x256x512x512 bf16)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
