"""Cost of the guarded Adam update (sgg_adam_guard, csrc/adam.hip) beside the plain one (sgg_adam_iter) on one MI355X.

    python tools/bench_guard.py [--warmup 5] [--runs 20] [--out profiles/guard_bench.txt]

At the flat-buffer sizes of the default generator and discriminator (module.ParamStore.numel): `warmup` untimed calls, then
`runs` calls each bracketed by its own pair of HIP events, of
  plain    sgg_adam_iter                         (2 launches: the 1-thread prep, the update)
  guarded  sgg_adam_guard, max_norm = 1          (3 launches: sum of squares, fold + decision, the update)
  sumsq    sgg_grad_sumsq alone                  (the extra pass)
once "cold" -- a 512 MiB buffer is rewritten before every timed call, so nothing of the four arrays is left in the 256 MiB
Infinity Cache, as after a backward pass -- and once "warm" (calls back to back).  The line reports the median, minimum and
maximum in us, and beside them the byte floors computed from the size alone at the 6.29 TB/s a float4 copy reaches on this
part: 4 bytes per element for the extra read of the gradient, 28 for the update (theta, m, v read and written, g read).
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sggan_amd import kernels as K
    from sggan_amd.module import ParamStore, discriminator_param_specs, generator_param_specs
    assert torch.cuda.is_available(), "bench_guard.py measures on the GPU"
    sizes = (("generator", ParamStore(generator_param_specs(), "cpu").numel), ("discriminator", ParamStore(discriminator_param_specs(), "cpu").numel))
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    lines = []
    for name, n in sizes:
        gen = torch.Generator().manual_seed(n % 1009)
        theta, g = torch.randn(n, generator=gen).cuda(), (torch.randn(n, generator=gen) * 0.1).cuda()
        m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        state = torch.zeros(2, dtype=torch.int64, device="cuda")
        guard = torch.zeros(4, dtype=torch.float64, device="cuda")
        ws = K.grad_guard_workspace(n, "cuda")
        calls = (("plain", lambda: K.adam_iter(theta, g, m, v, state, 2e-4, 0.5, 0.999, 1e-7)),
                 ("guarded", lambda: K.adam_guard(theta, g, m, v, state, guard, ws, None, 2e-4, 0.5, 0.999, 1e-7, 1.0, 1.0)),
                 ("sumsq", lambda: K.grad_sumsq(g, ws)))
        floor_pass, floor_update = 4.0 * n / HBM * 1e6, 28.0 * n / HBM * 1e6
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
                lines.append(f"{name} n = {n} {mode:4s} {kind:7s}: median {med[kind]:8.1f} us  min {min(us):8.1f}  max {max(us):8.1f}  "
                             f"({a.runs} runs after {a.warmup} warm-up)")
                print(lines[-1], flush=True)
            extra = med["guarded"] - med["plain"]
            lines.append(f"{name} n = {n} {mode:4s} guarded - plain = {extra:.1f} us = {extra / floor_pass:.2f} x the extra pass's byte floor "
                         f"({floor_pass:.1f} us = 4 B x n at 6.29 TB/s); the update's own floor is {floor_update:.1f} us (28 B x n)")
            print(lines[-1], flush=True)
        rec = guard.tolist()
        assert rec[2] == 0.0 and rec[3] == 2.0 * (a.warmup + a.runs) and 0.0 < rec[1] < 1.0, rec     # every guarded call clipped and applied
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
