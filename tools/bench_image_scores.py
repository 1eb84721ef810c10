"""Cost per test image of the paired image-quality score (metric.scores_image_fake, csrc/imgqual.hip) on one MI355X, beside the
generator's forward pass at the same size -- the work the test pass does per image before it scores it.

    python tools/bench_image_scores.py [--shapes 128x128,512x256] [--warmup 20] [--calls 200] [--rounds 7] [--out profiles/image_scores_bench.txt]

Per shape (H x W), one pair: a seeded blocky colour map plus noise as the generator's channel-padded bf16 output (1,H,W,8) in
[-1,1] against a uint8 (1,H,W,3) target.
  image scores : metric.scores_image_fake -- the two launches of sgg_image_quality plus the wrapper's two allocations
  (kernels)    : kernels.image_quality into a caller's output and workspace -- the two launches alone
  generator    : the default ResNet generator's forward (ngf 64, 9 blocks, bf16) on one image of that size, graph-free
Each figure is the time of one call as the test pass pays it, launches included: `calls` back-to-back calls between one pair of
HIP events, divided by `calls` (the generator: `calls` / 10); the paths alternate within a round and the line reports the
median, minimum and maximum over `rounds`.  There is no earlier implementation to compare with: the last line per shape gives
the score's share beside the forward pass.
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
    return {"fake_bf16": torch.as_tensor(fake).cuda().to(torch.bfloat16), "target_u8": torch.as_tensor(rgb[entry][None].astype(np.uint8)).cuda(),
            "photo": torch.as_tensor(rng.random((1, H, W, 3)).astype(np.float32)).cuda()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x128,512x256")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import sggan_amd
    from sggan_amd import kernels as K
    from sggan_amd import metric as M
    assert torch.cuda.is_available(), "needs a GPU"
    G = sggan_amd.Generator(dtype=torch.bfloat16)
    lines = []
    for shape in a.shapes.split(","):
        H, W = (int(v) for v in shape.split("x"))
        x = inputs(H, W)
        ws = torch.empty(K.image_quality_workspace_bytes(1, H, W), dtype=torch.uint8, device="cuda")
        out = torch.empty((1, 3), dtype=torch.float64, device="cuda")
        xi = G.to_internal(x["photo"])
        paths = {
            "image scores": (lambda: M.scores_image_fake(x["target_u8"], x["fake_bf16"]), a.calls),
            "image scores (kernels)": (lambda: K.image_quality(x["target_u8"], x["fake_bf16"], out=out, workspace=ws), a.calls),
            "generator forward": (lambda: G.forward(xi), max(a.calls // 10, 1)),
        }
        times = {k: [] for k in paths}
        for fn, calls in paths.values():
            for _ in range(min(a.warmup, calls)):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for name, (fn, calls) in paths.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / calls)          # us per call
        for name, (_, calls) in paths.items():
            med = statistics.median(times[name])
            lines.append(f"{H}x{W} {name}: median {med:.2f} us per image  min {min(times[name]):.2f}  max {max(times[name]):.2f}  "
                         f"({a.rounds} rounds of {calls} calls after {min(a.warmup, calls)} warm-up)")
            print(lines[-1], flush=True)
        share = statistics.median(times["image scores"]) / statistics.median(times["generator forward"])
        lines.append(f"{H}x{W}: image scores / generator forward = {share:.4f}")
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
