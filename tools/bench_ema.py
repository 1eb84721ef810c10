"""Cost of keeping the generator weight average (sgg_adam_ema, csrc/adam.hip) on one MI355X.

    python tools/bench_ema.py [--warmup 5] [--runs 20] [--steps 10] [--repeats 5] [--no-step] [--out profiles/ema_bench.txt]

Part 1, at the flat-buffer sizes of the two generator kinds (module.ParamStore.numel of the ResNet and of the U-Net): `warmup`
untimed calls, then `runs` calls each bracketed by its own pair of HIP events, of
  plain       sgg_adam_iter                                  (2 launches; 28 bytes per element)
  fused       sgg_adam_ema, guarded = 0                      (2 launches; 36 bytes per element)
  plain+lerp  sgg_adam_iter, then ema.lerp_(theta, 1 - d)    (3 launches; 28 + 12 bytes per element; d chosen on the host)
once "cold" -- a 512 MiB buffer is rewritten before every timed call, so nothing of the arrays is left in the 256 MiB Infinity
Cache, as after a backward pass -- and once "warm" (calls back to back).  Median, minimum and maximum in us, and beside them
the byte floors at the 6.29 TB/s a float4 copy reaches on this part.

Part 2, the step bench.py times (cycle mode, bf16, 256x512, batch 8, HIP-graph replay) built without and with ema_decay: after
`warmup` steps, `repeats` blocks of `steps` replayed steps per model, the two models taking turns block by block so that both
see the same machine state; ms per step of every block, and the medians and spreads of the two.
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import sggan_amd
    from sggan_amd import kernels as K
    from sggan_amd.module import ParamStore, generator_param_specs, unet_param_specs
    assert torch.cuda.is_available(), "bench_ema.py measures on the GPU"
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    sizes = (("resnet generator", ParamStore(generator_param_specs(), "cpu").numel), ("unet generator", ParamStore(unet_param_specs(), "cpu").numel))
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    decay = 0.999
    for name, n in sizes:
        gen = torch.Generator().manual_seed(n % 1009)
        theta, g = torch.randn(n, generator=gen).cuda(), (torch.randn(n, generator=gen) * 0.1).cuda()
        m, v, ema = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), theta.clone()
        state = torch.zeros(2, dtype=torch.int64, device="cuda")
        ema_state = torch.zeros(2, device="cuda")

        def plain():
            K.adam_iter(theta, g, m, v, state, 2e-4, 0.5, 0.999, 1e-7)

        def fused():
            K.adam_ema(theta, g, m, v, ema, state, ema_state, decay, None, 2e-4, 0.5, 0.999, 1e-7)

        def unfused():
            K.adam_iter(theta, g, m, v, state, 2e-4, 0.5, 0.999, 1e-7)
            ema.lerp_(theta, 1.0 - decay)

        calls = (("plain", plain), ("fused", fused), ("plain+lerp", unfused))
        floors = {"plain": 28.0 * n / HBM * 1e6, "fused": 36.0 * n / HBM * 1e6, "plain+lerp": 40.0 * n / HBM * 1e6}
        for mode in ("cold", "warm"):
            med = {}
            for kind, run in calls:
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
                med[kind] = statistics.median(us)
                say(f"{name} n = {n} {mode:4s} {kind:10s}: median {med[kind]:8.1f} us  min {min(us):8.1f}  max {max(us):8.1f}  "
                    f"byte floor {floors[kind]:6.1f} us  ({a.runs} runs after {a.warmup} warm-up)")
            say(f"{name} n = {n} {mode:4s} fused / plain = {med['fused'] / med['plain']:.3f} (36 / 28 = {36 / 28:.3f} by bytes);  "
                f"fused / (plain+lerp) = {med['fused'] / med['plain+lerp']:.3f} (36 / 40 = 0.900 by bytes);  "
                f"fused - plain = {med['fused'] - med['plain']:.1f} us")
        assert state[0].item() == 6 * (a.warmup + a.runs)
        del theta, g, m, v, ema
    del flush
    torch.cuda.empty_cache()

    if not a.no_step:
        from bench import set_inputs
        N, H, W = 8, 256, 512
        models = {}
        for tag, extra in (("without", {}), ("with ema", {"ema_decay": decay})):
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
            say(f"cycle step bf16 {H}x{W} batch {N}, graph replay, {tag:8s}: ms/step per block of {a.steps} " + " ".join(f"{x:.3f}" for x in xs) +
                f"  median {statistics.median(xs):.3f}  spread {(max(xs) - min(xs)) / statistics.median(xs) * 100:.2f} %")
        m0, m1 = statistics.median(ms["without"]), statistics.median(ms["with ema"])
        say(f"cycle step: with ema / without = {m1 / m0:.4f} ({(m1 - m0) * 1e3:+.1f} us per step, two generators)")
        gl, dl = models["with ema"].losses()
        assert abs(gl) < float("inf") and abs(dl) < float("inf")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
