"""Cost of the test pass's sliced Wasserstein distance (metric.SWD, csrc/swd.hip) on one MI355X: what ``add`` costs per image
and what the one-off ``result()`` costs per test set, beside the generator's forward pass at the same size -- the work the test
pass does per image before it scores it.

    python tools/bench_swd.py [--shape 512x256] [--images 6,500] [--warmup 5] [--runs 20] [--out profiles/swd_bench.txt]

The image pair is a seeded blocky colour map plus noise as the generator's channel-padded bf16 output (1,H,W,8) in [-1,1] (the
fake) against a uint8 (1,H,W,3) image (the real).  Per set size n:
  add        : metric.SWD.add of one pair -- two pyramids (2 x 2L launches) and 2 x L descriptor launches, default 128 patches
  result     : metric.SWD.result() over n pairs -- per level and repeat two projections (5 launches each), two sorts
               (torch.sort) and the distance launch, then the one read-back
  generator  : the default ResNet generator's forward (ngf 64, 9 blocks, bf16) on one image of that size, graph-free
Every figure is one call between a pair of HIP events (``result`` ends in its own read-back); the line reports the median,
minimum and maximum over ``runs`` calls after ``warmup`` untimed ones.  No target is set: there is no earlier implementation.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inputs(H, W, seed=0):
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (19, 3))
    blocks = rng.integers(0, 19, ((H + 7) // 8, (W + 7) // 8))
    entry = np.repeat(np.repeat(blocks, 8, axis=0), 8, axis=1)[:H, :W]
    colour = np.clip(np.rint(rgb[entry] + rng.normal(0.0, 6.0, (H, W, 3))), 0, 255)
    fake = np.zeros((1, H, W, 8), dtype=np.float32)
    fake[0, ..., :3] = (colour + 0.5) / 127.5 - 1.0
    real = np.clip(np.rint(rgb[entry] + rng.normal(0.0, 20.0, (H, W, 3))), 0, 255).astype(np.uint8)
    return {"fake_bf16": torch.as_tensor(fake).cuda().to(torch.bfloat16), "real_u8": torch.as_tensor(real[None]).cuda(),
            "photo": torch.as_tensor(rng.random((1, H, W, 3)).astype(np.float32)).cuda()}


def timed(fn, warmup, runs):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))                     # ms
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="512x256")
    ap.add_argument("--images", default="6,500")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import sggan_amd
    from sggan_amd import metric as M
    assert torch.cuda.is_available(), "needs a GPU"
    H, W = (int(v) for v in a.shape.split("x"))
    x = inputs(H, W)
    G = sggan_amd.Generator(dtype=torch.bfloat16)
    xi = G.to_internal(x["photo"])
    lines = []

    def report(name, ms, unit):
        lines.append(f"{H}x{W} {name}: median {statistics.median(ms):.3f} ms per {unit}  min {min(ms):.3f}  max {max(ms):.3f}  "
                     f"({a.runs} calls after {a.warmup} warm-up)")
        print(lines[-1], flush=True)

    fwd = timed(lambda: G.forward(xi), a.warmup, a.runs)
    report("generator forward", fwd, "image")
    for n in (int(v) for v in a.images.split(",")):
        s = M.SWD(H, W, n)

        def add_one():
            if s.count["fakes"] == n:                       # the buffers are full: start over (no allocation, no launch)
                s.count = {"fakes": 0, "reals": 0}
            s.add(x["fake_bf16"], x["real_u8"])

        add = timed(add_one, a.warmup, a.runs)
        s.count = {"fakes": 0, "reals": 0}
        for _ in range(n):
            s.add(x["fake_bf16"], x["real_u8"])
        res = timed(s.result, a.warmup, a.runs)
        report(f"n={n} add (one pair, {s.levels} levels, {s.patches} patches)", add, "image")
        report(f"n={n} result ({s.repeats} x {s.dirs_per_repeat} directions, M = {n * s.patches})", res, "test set")
        total = statistics.median(add) * n + statistics.median(res)
        lines.append(f"{H}x{W} n={n}: SWD per image (add + result / n) = {total / n:.3f} ms = {total / n / statistics.median(fwd):.4f} of a "
                     "generator forward")
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
