"""Cost of the discriminators' differentiable augmentation (csrc/diffaug.hip) on one MI355X.

    python tools/bench_diffaug.py [--warmup 5] [--runs 20] [--steps 10] [--repeats 5] [--no-step] [--out profiles/diffaug_bench.txt]

Part 1, at the shapes of the step bench.py times (cycle mode, bf16, 256x512, batch 8: the discriminators' stacked input has 32
rows, the generators' loss goes back through 16): `warmup` untimed calls, then `runs` calls each bracketed by its own pair of HIP
events, of
  draw      sgg_diffaug_draw, 8 rows                     (1 launch)
  forward   sgg_diffaug_fwd, 32 rows                     (2 launches; reads x twice, writes y: 3 x 16 bytes per pixel)
  backward  sgg_diffaug_bwd with an addend, 16 rows      (2 launches; reads dy twice and the addend, writes dx: 4 x 16 bytes)
once "cold" -- a 512 MiB buffer is rewritten before every timed call, so nothing is left in the 256 MiB Infinity Cache -- and
once "warm" (calls back to back).  Median, minimum and maximum in us, and beside them the byte floors at the 6.29 TB/s a float4
copy reaches on this part.

Part 2, that step built without and with diffaug="color,cutout", HIP-graph replay: after `warmup` steps, `repeats` blocks of
`steps` replayed steps per model, the two models taking turns block by block so that both see the same machine state; ms per step
of every block, and the medians and spreads of the two.
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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="part 1 only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffaug_bench.txt"), help="where the lines are written ('' : nowhere)")
    a = ap.parse_args()
    import torch
    import sggan_amd
    from sggan_amd import kernels as K
    assert torch.cuda.is_available(), "bench_diffaug.py measures on the GPU"
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    N, H, W = 8, 256, 512
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    it = torch.zeros(1, dtype=torch.int64, device="cuda")
    par = torch.empty((4 * N, 8), device="cuda")
    for i in range(4):
        K.diffaug_draw(par[i * N:(i + 1) * N], it, 19, 0, i, H, W, 3)
    x = torch.rand((4 * N, H, W, 8), device="cuda").to(torch.bfloat16)
    y = torch.empty_like(x)
    dy, addend = x[:2 * N], x[2 * N:]
    dx = y[:2 * N]
    px = H * W * 16
    calls = (("draw", lambda: K.diffaug_draw(par[:N], it, 19, 0, 0, H, W, 3), 0.0),
             ("forward", lambda: K.diffaug(x, par, 3, out=y), 3.0 * 4 * N * px),
             ("backward", lambda: K.diffaug_bwd(dy, par[N:3 * N], 3, addend=addend, out=dx), 4.0 * 2 * N * px))
    for mode in ("cold", "warm"):
        for kind, run, nbytes in calls:
            for _ in range(a.warmup):
                run()
            torch.cuda.synchronize()
            us = []
            for _ in range(a.runs):
                if mode == "cold":
                    flush.fill_(1)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            say(f"diffaug {kind:8s} bf16 {H}x{W} {mode:4s}: median {statistics.median(us):7.1f} us  min {min(us):7.1f}  max {max(us):7.1f}  "
                f"{nbytes / 1e6:6.1f} MB  byte floor {nbytes / HBM * 1e6:5.1f} us  ({a.runs} runs after {a.warmup} warm-up)")
    del flush, x, y
    torch.cuda.empty_cache()

    if not a.no_step:
        from bench import set_inputs
        models = {}
        for tag, extra in (("without", {}), ("with diffaug", {"diffaug": "color,cutout"})):
            mdl = sggan_amd.sggan(sggan_amd.default_args(dtype="bf16", image_height=H, image_width=W, batch_size=N, cycle=True, graph=True, **extra))
            set_inputs(mdl, N, H, W, 19)
            for _ in range(a.warmup):
                mdl.train_step()
            models[tag] = mdl
        torch.cuda.synchronize()
        ms = {tag: [] for tag in models}
        for rep in range(a.repeats):
            for tag, mdl in models.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    mdl.train_step()
                e1.record()
                e1.synchronize()
                ms[tag].append(e0.elapsed_time(e1) / a.steps)
        for tag, xs in ms.items():
            say(f"cycle step bf16 {H}x{W} batch {N}, graph replay, {tag:12s}: ms/step per block of {a.steps} " + " ".join(f"{v:.3f}" for v in xs) +
                f"  median {statistics.median(xs):.3f}  spread {(max(xs) - min(xs)) / statistics.median(xs) * 100:.2f} %")
        m0, m1 = statistics.median(ms["without"]), statistics.median(ms["with diffaug"])
        say(f"cycle step: with diffaug / without = {m1 / m0:.4f} ({(m1 - m0) * 1e3:+.1f} us per step: 4 draws, 2 + 2 launches over 32 + 16 images)")
        gl, dl = models["with diffaug"].losses()
        assert abs(gl) < float("inf") and abs(dl) < float("inf")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
