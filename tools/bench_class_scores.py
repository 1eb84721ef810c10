"""Cost per test image of the class-level score (metric.scores_class_fake, csrc/evalseg.hip) on one MI355X, beside the
reference-rule path it stands next to in the test pass.

    python tools/bench_class_scores.py [--shapes 128x128,512x256] [--warmup 20] [--calls 200] [--rounds 7] [--out profiles/class_scores_bench.txt]

Per shape (H x W), one image: a seeded blocky class map, its colours from a 19-entry palette plus noise as the generator's
channel-padded bf16 output (N,H,W,8) in [-1,1], n_class = 34.
  class scores : scores_class_fake(band_radius=3) -- the band launch + one fused decode-and-count launch into a device matrix
  (band 0)     : scores_class_fake(band_radius=0) -- the one fused launch
  reference    : argmax_u8_labels x 2 + confusion_hist -- the existing label rule on two f32 (N,H,W,3) images, three launches
Each figure is the time of one call as the test pass pays it, launches included: `calls` back-to-back calls between one pair of
HIP events, divided by `calls`; the paths alternate within a round and the line reports the median, minimum and maximum over
`rounds`.  Beside it: the bytes the path must move (computed from the shape) over that time.  Both are launch-latency sized at
these shapes, so the GB/s are far below what the memory system does; for the per-kernel split run the same command under
`rocprofv3 --kernel-trace --stats`.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_CLASS, K_PAL, BAND = 34, 19, 3


def inputs(H, W, seed=0):
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (K_PAL, 3))
    classes = rng.permutation(N_CLASS)[:K_PAL].astype(np.uint8)
    blocks = rng.integers(0, K_PAL, ((H + 7) // 8, (W + 7) // 8))
    entry = np.repeat(np.repeat(blocks, 8, axis=0), 8, axis=1)[:H, :W]
    colour = np.clip(np.rint(rgb[entry] + rng.normal(0.0, 6.0, (H, W, 3))), 0, 255)
    fake = np.zeros((1, H, W, 8), dtype=np.float32)
    fake[0, ..., :3] = (colour + 0.5) / 127.5 - 1.0
    seg = rng.random((1, H, W, 3)).astype(np.float32)
    keys = ((rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]).astype(np.uint32)
    return {"fake_bf16": torch.as_tensor(fake).cuda().to(torch.bfloat16), "truth": torch.as_tensor(classes[entry][None]).cuda(),
            "palette": (keys, classes), "seg_f32": torch.as_tensor(seg).cuda(),
            "fake_f32": torch.as_tensor(fake[..., :3].copy()).cuda()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x128,512x256")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sggan_amd import metric as M
    assert torch.cuda.is_available(), "needs a GPU"
    lines = []
    for shape in a.shapes.split(","):
        H, W = (int(v) for v in shape.split("x"))
        x = inputs(H, W)
        hist = torch.zeros((N_CLASS, N_CLASS), dtype=torch.int64, device="cuda")
        flat = hist.view(-1)

        def reference():
            lt, lp = M.argmax_u8_labels(x["seg_f32"]), M.argmax_u8_labels(x["fake_f32"])
            M._accumulate_hist(flat, lt, lp, N_CLASS)

        P = H * W
        paths = {
            "class scores (band 3)": (lambda: M.scores_class_fake(x["truth"], x["fake_bf16"], N_CLASS, x["palette"], band_radius=BAND, hist=hist),
                                      P * (16 + 1 + 1) + P * (1 + 1)),          # decode: pixel, truth, select; band: read + write
            "class scores (band 0)": (lambda: M.scores_class_fake(x["truth"], x["fake_bf16"], N_CLASS, x["palette"], hist=hist), P * (16 + 1)),
            "reference rule": (reference, P * (2 * 12 + 2 * 4 + 2 * 4)),        # two f32 images in, two int32 label maps out and in again
        }
        times = {k: [] for k in paths}
        for fn, _ in paths.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for name, (fn, _) in paths.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)          # us per call
        for name, (_, nbytes) in paths.items():
            med = statistics.median(times[name])
            lines.append(f"{H}x{W} {name}: median {med:.2f} us per image  min {min(times[name]):.2f}  max {max(times[name]):.2f}  "
                         f"({a.rounds} rounds of {a.calls} calls after {a.warmup} warm-up)  bytes {nbytes}  -> {nbytes / med / 1e3:.2f} GB/s")
            print(lines[-1], flush=True)
        ratio = statistics.median(times["reference rule"]) / statistics.median(times["class scores (band 3)"])
        lines.append(f"{H}x{W}: reference rule / class scores (band 3) = {ratio:.2f}")
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
