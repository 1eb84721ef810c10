"""Cost of the device-resident input pipeline beside the step it feeds (one MI355X).

Cycle step, bf16, 512x256, batch 8, HIP-graph replay, one model, one process:
  (a) inputs staged once and reused                     -- the configuration bench.py times
  (b) a fresh DirectoryBatches batch before every step  -- 16 images + 16 colour labels of 2048x1024 resampled per step
in interleaved blocks (a b a b ...), warm-up excluded, each block bracketed by a device synchronise and timed on the host
clock.  Requires (b) >= 0.98 x (a) (exit status 1 otherwise).  Also times the loader alone (HIP events around fills).

    python tools/bench_data.py [--blocks 6] [--steps 10] [--samples 100] [--out profiles/data_pipeline.txt]
    python tools/bench_data.py --fills 20        # loader only: the run to put under rocprofv3 --kernel-trace --stats
    python tools/bench_data.py --augment --batch 4 [--out profiles/data_pipeline_augment.txt]

--augment: the loader yields every sample plus its augmented copy (DirectoryBatches(augment=True): sgg_warp_affine_u8 +
sgg_resample_f32 per copy), so --batch 4 feeds the step the usual 8 images per domain.  The ratio (b) / (a) is reported, not
required: its yardstick is the plain loader's ratio from a run without --augment in the same session.

The 100-sample cache replicates the Cityscapes fixture crops (tests/golden/city_small, 1024x512) 2 x 2 into full 2048x1024
sources, so every sample costs the bytes a Cityscapes file does.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--fills", type=int, default=0, help="loader only: this many fills, no training step")
    ap.add_argument("--augment", action="store_true", help="doubled batches: every sample plus its augmented copy")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import sggan_amd
    from sggan_amd import data as D
    dev = "cuda:0"
    fix = D.DatasetCache(os.path.join(ROOT, "tests", "golden", "city_small"), "trainA", device="cpu")
    big = lambda t: np.tile(t.numpy(), (2, 2) + (1,) * (t.dim() - 2))
    n_fix = len(fix)
    imgs = [big(fix.stacks[fix.image[i % n_fix][0]][fix.image[i % n_fix][1]]) for i in range(n_fix)]
    labs = [big(fix.stacks[fix.label[i % n_fix][0]][fix.label[i % n_fix][1]]) for i in range(n_fix)]
    clss = [big(fix.stacks[fix.classmap[i % n_fix][0]][fix.classmap[i % n_fix][1]]) for i in range(n_fix)]
    rep = lambda xs: [xs[i % n_fix] for i in range(a.samples)]
    cache_A = D.DatasetCache.from_arrays(rep(imgs), rep(labs), rep(clss), device=dev)
    cache_B = D.DatasetCache.from_arrays(rep(imgs[::-1]), rep(labs[::-1]), rep(clss[::-1]), device=dev)
    args = sggan_amd.default_args(dtype="bf16", device=dev, image_height=a.height, image_width=a.width, batch_size=a.batch,
                                  cycle=True, graph=True, train_size=10 ** 8)
    model = sggan_amd.sggan(args)
    batches = D.DirectoryBatches(model, args, cache_A, cache_B, augment=a.augment)
    per_step = a.batch * (2 if a.augment else 1)              # images per domain the step sees

    def stream():
        ep = 0
        while True:
            for b in batches(ep):
                yield b
            ep += 1
    fresh = stream()
    src_bytes = sum(int(np.prod(k[1:])) for d in batches.domains for k in (d.cache.image[0][0], d.cache.label[0][0])) * a.batch
    out_bytes = 4 * per_step * a.height * a.width * 8 * 2
    if a.augment:       # a copy reads its source again and writes + reads the f32 (S, S, 4) intermediate
        inter = sum(16 * k[1] * k[1] for d in batches.domains for k in (d.cache.image[0][0], d.cache.label[0][0])) * a.batch
        src_bytes = 2 * src_bytes + 2 * inter
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    say(f"bench_data: cycle step bf16 {a.width}x{a.height} batch {a.batch}{' + augmented copies (step batch %d)' % per_step if a.augment else ''}, graph replay; cache {a.samples} samples/domain of "
        f"{imgs[0].shape[1]}x{imgs[0].shape[0]}; loader reads {src_bytes / 1e6:.1f} MB and writes {out_bytes / 1e6:.1f} MB per step")

    # loader alone
    n_fill = a.fills or 30
    for _ in range(3):
        next(fresh)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n_fill):
        next(fresh)
    e1.record()
    t_host = (time.perf_counter() - t0) / n_fill
    torch.cuda.synchronize()
    fill_ms = e0.elapsed_time(e1) / n_fill
    say(f"loader alone: {fill_ms * 1e3:.1f} us per step's batch on the device ({(src_bytes + out_bytes) / fill_ms / 1e6:.1f} GB/s), "
        f"{t_host * 1e6:.1f} us of host time to enqueue it")
    result = {"fill_us": fill_ms * 1e3, "fill_host_us": t_host * 1e6, "fill_GBps": (src_bytes + out_bytes) / fill_ms / 1e6}
    if not a.fills:
        for k, v in next(fresh).items():
            setattr(model, k, v)
        for _ in range(a.warmup):
            model.train_step()
        torch.cuda.synchronize()
        times = {"a": [], "b": []}
        for blk in range(a.blocks):
            for mode in ("a", "b"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    if mode == "b":
                        next(fresh)
                    model.train_step()
                torch.cuda.synchronize()
                times[mode].append((time.perf_counter() - t0) / a.steps)
        gl, dl = model.losses()
        assert np.isfinite(gl) and np.isfinite(dl)
        ips = {m: per_step / statistics.median(v) for m, v in times.items()}
        for m, what in (("a", "inputs staged once"), ("b", "fresh batch every step")):
            say(f"({m}) {what}: {ips[m]:.1f} images/s  (median of {a.blocks} blocks of {a.steps} steps; ms/step per block: "
                + " ".join(f"{1e3 * t:.3f}" for t in times[m]) + ")")
        ratio = ips["b"] / ips["a"]
        say(f"(b) / (a) = {ratio:.4f}  " + ("(reported; compare with the plain loader's ratio of the same session)" if a.augment else "(required >= 0.98)"))
        result.update({"a_images_per_sec": ips["a"], "b_images_per_sec": ips["b"], "ratio": ratio, "pass": a.augment or ratio >= 0.98})
    print(json.dumps(result))
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if result.get("pass", True) else 1


if __name__ == "__main__":
    sys.exit(main())
