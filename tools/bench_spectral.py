"""Cost of spectral-norm discriminators (--d_norm spectral; csrc/spectral.hip) on one MI355X.

    python tools/bench_spectral.py [--warmup 5] [--runs 20] [--steps 20] [--out profiles/spectral_bench.txt]
    python tools/bench_spectral.py --count

Per discriminator, at full width (ndf 64, 8.79 M kernel elements, the largest layer 4608 x 512): `warmup` untimed calls, then
`runs` calls each bracketed by its own pair of HIP events, of
  sigma    sgg_spectral_sigma                       (2 launches: the banded pass over every kernel, the fold)
  pack     sgg_pack_conv_weights_batch_scaled       (1 launch), beside the plain sgg_pack_conv_weights_batch it replaces
  grad     sgg_spectral_grad                        (2 launches: the dot, the in-place transform)
once "cold" -- a 512 MiB buffer is rewritten before every timed call, as after a backward pass -- and once "warm".  Then the
cycle step at 512 x 256, batch 8, bf16, replayed from its recording, with the option off and on, alternately, `steps` steps a leg.

--count prints the launches a default model captures (the discriminator's forward + backward, the reference step, the cycle
step) at the size tests/test_gpu_spectral.py pins them at; it uses nothing of the option, so it runs on older trees as well.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def captured_nodes(device, body):
    """Nodes a recording of ``body`` captures (sgg_stream_capture_nodes, asked before every segment is closed)."""
    import torch
    from sggan_amd import _abi as A, kernels as K
    from sggan_amd.graph import StepProgram

    class Counting(StepProgram):
        nodes = 0

        def _close(self):
            n = C.c_int(0)
            A.check(A.lib().sgg_stream_capture_nodes(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), C.byref(n)), "nodes")
            self.nodes += n.value
            super()._close()

    prog = Counting(device)
    K._RECORDER = prog
    try:
        prog.record(body)
    finally:
        K._RECORDER = None
    return prog.nodes


def rand_inputs(N, H, W, mask_hw, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    real, seg = torch.rand((N, H, W, 3), generator=g), torch.rand((N, H, W, 3), generator=g)
    mask = torch.nn.functional.one_hot(torch.randint(0, 34, (N,) + tuple(mask_hw), generator=g), 34).float()
    return real, seg, mask


def default_model_counts(**kw):
    """{"D", "reference", "cycle"}: captured launches of a model at 2 x 128 x 128, bf16, ngf = ndf = 8, n_blocks = 1."""
    import torch
    import sggan_amd
    out = {}
    for cycle in (False, True):
        m = sggan_amd.sggan(sggan_amd.default_args(ngf=8, ndf=8, n_blocks=1, dtype="bf16", cycle=cycle, **kw))
        m.real_A, m.seg_A, m.mask_A = rand_inputs(2, 128, 128, (4, 4), 40)
        if cycle:
            m.real_B, m.seg_B, m.mask_B = rand_inputs(2, 128, 128, (4, 4), 50)
        m.train_step()
        m._stage_inputs()                        # (device-resident inputs, as a recorded step reads them: no copy inside the capture)
        torch.cuda.synchronize()
        out["cycle" if cycle else "reference"] = captured_nodes(m.device, m._step_body)
        if not cycle:
            D = m.discriminator
            x, mask = m._prep(m.real_A), m._convert_input("mask_A", m.mask_A)
            d = torch.ones((2, 4, 4, 1), device="cuda")
            one = lambda: D.backward(D.forward(x, mask)[1], d, want_dx=True)
            one()
            torch.cuda.synchronize()
            out["D"] = captured_nodes(m.device, one)
    return out


def timed(run, warmup, runs, flush=None):
    import torch
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    us = []
    for _ in range(runs):
        if flush is not None:
            flush.fill_(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="skip the cycle-step legs (profiling the three launches)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_spectral.py measures on the GPU"
    if a.count:
        print(json.dumps(default_model_counts()))
        return
    import sggan_amd
    from sggan_amd import kernels as K
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    # ---- the three launches, per discriminator
    D = sggan_amd.Discriminator(norm="spectral", dtype=torch.bfloat16)
    D.P.grad.normal_()
    D.repack_all(torch.bfloat16)
    table, n, max_elems, _ = D._pack_tables[torch.bfloat16]
    sn = D._sn
    elems = sum(r * k for r, k in sn.mats)
    say(f"discriminator ndf = 64: {elems} kernel elements in {len(sn.mats)} layers, largest {max(sn.mats)}; bytes: sigma reads {4 * elems / 1e6:.1f} MB, "
        f"grad reads {8 * elems / 1e6:.1f} MB and writes {4 * elems / 1e6:.1f} MB")
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    calls = (("sigma", lambda: K.spectral_sigma(sn.table)),
             ("pack scaled", lambda: K.repack_batch(table, n, max_elems, torch.bfloat16, scale=sn.inv_sigma)),
             ("pack plain", lambda: K.repack_batch(table, n, max_elems, torch.bfloat16)),
             ("grad", lambda: K.spectral_grad(sn.table)))
    for mode in ("cold", "warm"):
        med = {}
        for kind, run in calls:
            us = timed(run, a.warmup, a.runs, flush if mode == "cold" else None)
            med[kind] = statistics.median(us)
            say(f"{mode:4s} {kind:11s}: median {med[kind]:7.1f} us  min {min(us):7.1f}  max {max(us):7.1f}  ({a.runs} runs after {a.warmup} warm-up)")
        say(f"{mode:4s} per discriminator and step: sigma + (pack scaled - pack plain) + grad = "
            f"{med['sigma'] + med['pack scaled'] - med['pack plain'] + med['grad']:.1f} us")
    del flush
    if a.kernels_only:
        return

    # ---- the cycle step, option off and on, alternately
    def model(kind):
        m = sggan_amd.sggan(sggan_amd.default_args(dtype="bf16", image_height=256, image_width=512, batch_size=8, cycle=True, graph=True, d_norm=kind))
        mhw = m.discriminator.out_hw(256, 512)
        m.real_A, m.seg_A, m.mask_A = rand_inputs(8, 256, 512, mhw, 1)
        m.real_B, m.seg_B, m.mask_B = rand_inputs(8, 256, 512, mhw, 2)
        for _ in range(a.warmup):
            m.train_step()
        torch.cuda.synchronize()
        return m
    models = {kind: model(kind) for kind in ("instance", "spectral")}
    ms = {kind: [] for kind in models}
    for _ in range(a.rounds):
        for kind, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                m.train_step()
            torch.cuda.synchronize()
            ms[kind].append((time.perf_counter() - t0) / a.steps * 1e3)
    for kind, v in ms.items():
        say(f"cycle step 512x256 batch 8 bf16, replayed, --d_norm {kind:8s}: {statistics.median(v):.3f} ms/step "
            f"(legs of {a.steps} steps, alternating: {', '.join('%.3f' % x for x in v)})")
    assert all(all(x == x for x in m.losses()) for m in models.values())
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
