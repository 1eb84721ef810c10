"""Cost of the feature-matching option of the paired step (csrc/featmatch.hip) on one MI355X.

    python tools/bench_featmatch.py [--warmup 3] [--runs 20] [--steps 10] [--repeats 3] [--no-step] [--out profiles/featmatch_bench.txt]

Part 1, sgg_feature_match alone (its two launches), bf16, on seven pairs shaped like the discriminator's features of the step at
512x256, batch 8, ndf 64: `warmup` untimed calls, then `runs` calls each bracketed by its own pair of HIP events, once "cold" -- a
512 MiB buffer is rewritten before every timed call, so nothing is left in the 256 MiB Infinity Cache -- and once "warm" (calls back
to back; in the step the features were written shortly before).  Median, minimum and maximum in us beside the byte floor of the
algorithm -- 3x the bytes of the seven fake-feature tensors: real and fake read once, the gradient written once -- at the 6.29 TB/s
a float4 copy reaches on this part.

Part 2, the reference step, bf16, 512x256, batch 8, HIP-graph replay, built without the option and with --fm_lambda 10: per leg a
fresh model, `warmup` steps, then `steps` replayed steps between two HIP events and the leg's peak device memory; the legs take turns
(`repeats` rounds) so that both see the same machine state."""
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="part 1 only")
    ap.add_argument("--no-kernel", action="store_true", help="part 2 only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "featmatch_bench.txt"), help="where the lines are written ('' : nowhere)")
    a = ap.parse_args()
    import torch
    import sggan_amd
    from sggan_amd import kernels as K
    assert torch.cuda.is_available(), "bench_featmatch.py measures on the GPU"
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    N, H, W = 8, 256, 512
    if not a.no_kernel:
        D = sggan_amd.Discriminator(df_dim=64, dtype=torch.bfloat16, device="cuda")
        x = torch.rand((2 * N, H, W, 3), device="cuda")
        mh, mw = D.out_hw(H, W)
        _, tape = D.forward(D.to_internal(x), torch.zeros((2 * N, mh, mw, D.segment_class), device="cuda"))
        reals, fakes = [t.clone() for t in D.features(tape, 0, N)], [t.clone() for t in D.features(tape, N, 2 * N)]
        crs = [u.cout for u in D.units]
        del tape
        grads = [torch.empty_like(f) for f in fakes]
        loss, term = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
        nbytes = 3.0 * sum(f.numel() * 2 for f in fakes)
        say("feature shapes: " + " ".join("x".join(map(str, f.shape)) for f in fakes) + f"; {sum((f.numel() // f.shape[-1] * (f.shape[-1] // 8) + K.FEATMATCH_CHUNK - 1) // K.FEATMATCH_CHUNK for f in fakes)} blocks")
        flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
        call = lambda: K.feature_match(reals, fakes, crs, loss, term, 10.0, out=grads)
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
            say(f"feature_match bf16, 7 pairs of the step at {H}x{W} batch {N}, {state:4s}: median {med:7.1f} us  min {min(us):7.1f}  max {max(us):7.1f}  "
                f"{nbytes / 1e6:7.1f} MB  byte floor {floor:6.1f} us  median / floor {med / floor:.2f}  {nbytes / med / 1e6:.2f} TB/s  "
                f"(both launches; {a.runs} runs after {a.warmup} warm-up)")
        del flush, reals, fakes, grads, D
        torch.cuda.empty_cache()

    if not a.no_step:
        from tools.bench_unet import inputs
        tags = (("off", {}), ("--fm_lambda 10", {"fm_lambda": 10.0}))
        ms, peak = {t: [] for t, _ in tags}, {t: 0 for t, _ in tags}
        for rep in range(a.repeats):
            for tag, kw in tags:
                torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
                mdl = sggan_amd.sggan(sggan_amd.default_args(dtype="bf16", image_height=H, image_width=W, batch_size=N, graph=True, **kw))
                mdl.real_A, mdl.seg_A, mdl.mask_A = inputs(mdl, N, H, W, 1)
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
        for tag, _ in tags:
            xs = ms[tag]
            say(f"reference step bf16 {H}x{W} batch {N}, graph replay, {tag:14s}: ms/step per leg of {a.steps} " + " ".join(f"{v:.3f}" for v in xs) +
                f"  median {statistics.median(xs):.3f}  spread {max(xs) - min(xs):.3f}  peak device memory {peak[tag] / 2**30:.2f} GiB")
        m0, m1 = statistics.median(ms["off"]), statistics.median(ms["--fm_lambda 10"])
        say(f"reference step: --fm_lambda 10 / off = {m1 / m0:.4f} ({m1 - m0:+.3f} ms per step, {(peak['--fm_lambda 10'] - peak['off']) / 2**30:+.2f} GiB peak; "
            "two more launches and seven addends in the generator-gradient walk through D)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
