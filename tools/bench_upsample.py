"""Cost of the resize-convolution option of generator_resnet (csrc/upsample.hip) on one MI355X.

    python tools/bench_upsample.py [--warmup 3] [--runs 20] [--steps 10] [--repeats 2] [--no-step] [--out profiles/upsample_bench.txt]

Part 1, sgg_upsample2x_fwd / sgg_upsample2x_bwd alone, bf16, both modes, at the inputs of d1 and d2 of the step at 512x256, batch 8 --
(8,64,128,256) and (8,128,256,128): `warmup` untimed calls, then `runs` calls each bracketed by its own pair of HIP events, once "cold"
-- a 512 MiB buffer is rewritten before every timed call, so nothing is left in the 256 MiB Infinity Cache -- and once "warm" (calls
back to back).  Median, minimum and maximum in us beside the byte floor of the algorithm -- every byte once: 5x the low-resolution
tensor per launch (the forward reads 1x and writes 4x, the adjoint reads 4x and writes 1x) -- at the 6.29 TB/s a float4 copy reaches
on this part.  The yardstick is this project's own streaming kernel, sgg_dropout: 1.21x its floor (profiles/dropout_bench.txt).

Part 2, the cycle step (paired, the configuration bench.py times) and the reference step, bf16, 512x256, batch 8, HIP-graph replay,
built with --upsample deconv, nearest and bilinear: per leg a fresh model, `warmup` steps, then `steps` replayed steps between two
HIP events and the leg's peak device memory; the legs take turns (`repeats` rounds) so that all see the same machine state.  Then the
multiply-adds of d1 + d2 either way, from the shapes."""
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
    ap.add_argument("--no-kernel", action="store_true", help="part 2 only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample_bench.txt"), help="where the lines are written ('' : nowhere)")
    a = ap.parse_args()
    import torch
    import sggan_amd
    from sggan_amd import kernels as K
    assert torch.cuda.is_available(), "bench_upsample.py measures on the GPU"
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    N, H, W = 8, 256, 512
    layers = (("d1", (N, H // 4, W // 4, 256), 128), ("d2", (N, H // 2, W // 2, 128), 64))
    if not a.no_kernel:
        flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
        for layer, shape, _ in layers:
            x = torch.randn(shape, device="cuda").to(torch.bfloat16)
            dy = torch.randn((shape[0], 2 * shape[1], 2 * shape[2], shape[3]), device="cuda").to(torch.bfloat16)
            y, dx = torch.empty_like(dy), torch.empty_like(x)
            nbytes = 5.0 * x.numel() * 2
            for mode in ("nearest", "bilinear"):
                for what, call in (("forward", lambda: K.upsample2x(x, mode, out=y)), ("adjoint", lambda: K.upsample2x_bwd(dy, mode, out=dx))):
                    for state in ("cold", "warm"):
                        for _ in range(a.warmup):
                            call()
                        torch.cuda.synchronize()
                        us = []
                        for _ in range(a.runs):
                            if state == "cold":
                                flush.fill_(1)
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            call()
                            e1.record()
                            e1.synchronize()
                            us.append(e0.elapsed_time(e1) * 1e3)
                        med, floor = statistics.median(us), nbytes / HBM * 1e6
                        say(f"upsample2x bf16 {layer} {'x'.join(map(str, shape))} {mode:8s} {what} {state:4s}: median {med:7.1f} us  min {min(us):7.1f}  "
                            f"max {max(us):7.1f}  {nbytes / 1e6:7.1f} MB  byte floor {floor:6.1f} us  median / floor {med / floor:.2f}  "
                            f"{nbytes / med / 1e6:.2f} TB/s  ({a.runs} runs after {a.warmup} warm-up)")
            del x, dy, y, dx
        del flush
        torch.cuda.empty_cache()

    if not a.no_step:
        from tools.bench_unet import inputs
        tags = ("deconv", "nearest", "bilinear")
        for cycle in (True, False):
            name = "cycle step (paired)" if cycle else "reference step"
            ms, peak = {t: [] for t in tags}, {t: 0 for t in tags}
            for rep in range(a.repeats):
                for tag in tags:
                    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
                    mdl = sggan_amd.sggan(sggan_amd.default_args(dtype="bf16", image_height=H, image_width=W, batch_size=N, cycle=cycle, graph=True,
                                                                 upsample=tag))
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
                    peak[tag] = max(peak[tag], torch.cuda.max_memory_allocated())
                    gl, dl = mdl.losses()
                    assert abs(gl) < float("inf") and abs(dl) < float("inf")
                    del mdl
                    torch.cuda.empty_cache()
            for tag in tags:
                xs = ms[tag]
                say(f"{name} bf16 {H}x{W} batch {N}, graph replay, --upsample {tag:8s}: ms/step per leg of {a.steps} " + " ".join(f"{v:.3f}" for v in xs) +
                    f"  median {statistics.median(xs):.3f}  spread {max(xs) - min(xs):.3f}  peak device memory {peak[tag] / 2**30:.2f} GiB")
            m0 = statistics.median(ms["deconv"])
            for tag in tags[1:]:
                m1 = statistics.median(ms[tag])
                say(f"{name}: --upsample {tag} / deconv = {m1 / m0:.4f} ({m1 - m0:+.3f} ms per step, {(peak[tag] - peak['deconv']) / 2**30:+.2f} GiB peak; "
                    f"{4 if cycle else 1} generator application(s), each 2 resampling and 2 adjoint launches and two convs of 4x the multiply-adds)")
    # the two layers' multiply-adds, forward, per generator application (backward: the same again for the data gradient and for the weight gradient)
    mac_t = sum(s[0] * s[1] * s[2] * 9 * s[3] * k for _, s, k in layers)
    say(f"d1 + d2 multiply-adds per application, forward, batch {N} at {H}x{W}: transposed stride-2 3x3 {mac_t / 1e9:.1f} G "
        f"(9 taps per INPUT pixel), resize-convolution {4 * mac_t / 1e9:.1f} G (9 taps per OUTPUT pixel: 4x); "
        f"the four 2x2 phase convs that nearest is equivalent to would take {16 / 9 * mac_t / 1e9:.1f} G (16/9x; not built)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
