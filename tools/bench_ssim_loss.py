"""Cost of the structural-similarity training loss (csrc/ssimloss.hip) on one MI355X.

    python tools/bench_ssim_loss.py [--warmup 5] [--runs 20] [--steps 10] [--repeats 5] [--no-step] [--out profiles/ssim_loss_bench.txt]

Part 1, at the shape of the step bench.py times (cycle mode, bf16, 256x512, batch 8, three colour channels; the step makes two
such calls): `warmup` untimed calls, then `runs` calls each bracketed by its own pair of HIP events, of
  loss      sgg_ssim_loss without dx                  (2 launches: forward, fold)
  loss+dx   sgg_ssim_loss accumulating into dx        (3 launches: forward writes the three coefficient maps as doubles, fold,
                                                       adjoint reads them with their halo and joins the gradient into dx)
once "cold" -- a 512 MiB buffer is rewritten before every timed call, so nothing is left in the 256 MiB Infinity Cache -- and
once "warm" (calls back to back).  Median, minimum and maximum in us, and beside them the bytes the call must move (operands,
the coefficient maps written and read once, dx read and written) with their floor at the 6.29 TB/s a float4 copy reaches.

Part 2, that step built without and with ssim_lambda=2, HIP-graph replay: after `warmup` steps, `repeats` blocks of `steps`
replayed steps per model, the two models taking turns block by block so that both see the same machine state; ms per step of
every block, and the medians and spreads of the two.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_loss_bench.txt"), help="where the lines are written ('' : nowhere)")
    a = ap.parse_args()
    import torch
    import sggan_amd
    from sggan_amd import _abi as A
    from sggan_amd import kernels as K
    assert torch.cuda.is_available(), "bench_ssim_loss.py measures on the GPU"
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    N, H, W, C = 8, 256, 512, 3
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    t = torch.rand((N, H, W, 8), device="cuda").to(torch.bfloat16)
    x = torch.rand((N, H, W, 8), device="cuda").to(torch.bfloat16)
    dx = torch.zeros_like(x)
    loss = torch.zeros(1, device="cuda")
    ws_bytes = int(A.lib().sgg_ssim_loss_workspace(N, H, W, C))
    coef = N * C * 3 * (H - 10) * (W - 10) * 8
    px = N * H * W * 16
    say(f"ssim_loss workspace at {N}x{H}x{W}x{C}: {ws_bytes} bytes ({ws_bytes / 1e6:.1f} MB, {coef / 1e6:.1f} MB of it the coefficient maps)")
    calls = (("loss", lambda: K.ssim_loss(t, x, C, loss, None, weight=2.0), 2.0 * px),
             ("loss+dx", lambda: K.ssim_loss(t, x, C, loss, dx, weight=2.0, accumulate_grad=True), 6.0 * px + 2.0 * coef))
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
            say(f"ssim_loss {kind:8s} bf16 {H}x{W} batch {N} {mode:4s}: median {statistics.median(us):7.1f} us  min {min(us):7.1f}  max {max(us):7.1f}  "
                f"{nbytes / 1e6:6.1f} MB  byte floor {nbytes / HBM * 1e6:5.1f} us  ({a.runs} runs after {a.warmup} warm-up)")
    del flush, t, x, dx
    torch.cuda.empty_cache()

    if not a.no_step:
        from bench import set_inputs
        models = {}
        for tag, extra in (("without", {}), ("with ssim_lambda", {"ssim_lambda": 2.0})):
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
            say(f"cycle step bf16 {H}x{W} batch {N}, graph replay, {tag:16s}: ms/step per block of {a.steps} " + " ".join(f"{v:.3f}" for v in xs) +
                f"  median {statistics.median(xs):.3f}  spread {(max(xs) - min(xs)) / statistics.median(xs) * 100:.2f} %")
        m0, m1 = statistics.median(ms["without"]), statistics.median(ms["with ssim_lambda"])
        say(f"cycle step: with ssim_lambda / without = {m1 / m0:.4f} ({(m1 - m0) * 1e3:+.1f} us per step: 2 calls of 3 launches over 8 images each)")
        gl, dl = models["with ssim_lambda"].losses()
        assert abs(gl) < float("inf") and abs(dl) < float("inf")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
