"""The Adam family (csrc/adam.hip) against bits recorded once, on the commit BEFORE the family was folded into one prep kernel,
one scalar update kernel and one launch path: every entry point, three steps each, at the edges of the three walks (the scalar
grid-stride update, the 2 048-element chunks of the update with the average, the 8 192-element chunks of the sum of squares).

tests/golden/adam_bits.json holds one SHA-256 per path, size and tensor (tests/golden/make_adam_bits.py wrote it, with the
functions of this module; the library under test never regenerates it).  A digest covers the tensor's raw bytes after step
1, step 2 and step 3, in that order, so a failure names the path, the size and the tensor that moved.  No tolerance: the
bitwise tests of test_gpu_ema.py / test_gpu_grad_guard.py / test_gpu_lr_schedule.py compare entry points with each other,
which says little once they share their kernels; this one compares them with what they computed before.

The inputs are a closed-form integer hash of (stream, index) mapped to f32 -- no library random generator, so the fixture
depends on the kernels and on nothing else.  The last test counts the launches of each path in a stream capture."""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_bits.json")
LR, B1, B2, EPS = 2e-4, 0.5, 0.999, 1e-7
# tail only / one 16-byte group / group + tail / around the 1 024 elements one round of a block's 16-byte groups covers / around
# one and four chunks of the update with the average (2 048) / around one chunk of the sum of squares (8 192) / whole chunks and a
# tail of either / 2 048 blocks of 256 and 257 more: the scalar update's grid is capped there and its threads take a second round
SIZES = [1, 3, 4, 5, 1023, 1024, 1028, 2044, 2048, 2052, 8191, 8192, 8193, 3 * 2048 + 13, 2 * 8192 + 7, 2048 * 256 + 257]
SCHED = (1, 1, 4)                     # steps_per_epoch, epoch_step, epochs: the third step runs at 2/3 of the rate
MAX_NORM = 2.0 ** -12                 # under every gradient's norm below: each guarded step with it is clipped
EMA_DECAY = 0.3                       # d_t = min(0.3, (1 + t) / (10 + t)): the ramp at t = 1, 2, the decay at t = 3
NAN_AT = 2                            # (1-based) step whose gradient carries one NaN

# path -> (entry, options).  The guarded variants are the same five for adam_guard and adam_ema.
_GUARDED = {"off": {}, "clip": {"max_norm": MAX_NORM}, "nan": {"nan": True}, "sched": {"sched": True, "max_norm": MAX_NORM},
            "scale": {"grad_scale": 0.125, "max_norm": MAX_NORM}}
PATHS = {"adam": ("adam", {}), "adam_iter": ("iter", {}), "adam_sched": ("sched", {"sched": True, "grad_scale": 0.5}),
         **{f"adam_guard/{k}": ("guard", o) for k, o in _GUARDED.items()},
         "adam_ema/plain": ("ema", {}),
         **{f"adam_ema/guard_{k}": ("ema", {"guarded": True, **o}) for k, o in _GUARDED.items()}}


def hashed_f32(stream, n):
    """n floats in [-1, 1), each a multiple of 2^-22: element i of stream s is a 32-bit mix of (s, i), its top 23 bits read as an
    integer.  Integer arithmetic only (uint64, masked to 32 bits); the conversion to f32 is exact."""
    M = np.uint64(0xFFFFFFFF)
    h = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B1) + np.uint64(stream) * np.uint64(0x85EBCA77) + np.uint64(1)) & M
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & M
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & M
    h ^= h >> np.uint64(15)
    return ((h >> np.uint64(9)).astype(np.int64) - (1 << 22)).astype(np.float32) / np.float32(1 << 22)


@functools.lru_cache(maxsize=None)
def problem(n):
    """theta0, ema0, three gradients (in [-1/8, 1/8)) and the second gradient with a NaN in the middle: device tensors, made once
    per size and never written."""
    theta0, ema0 = hashed_f32(1, n), hashed_f32(2, n)
    grads = [hashed_f32(3 + k, n) * np.float32(0.125) for k in range(3)]
    bad = grads[NAN_AT - 1].copy()
    bad[n // 2] = np.float32("nan")
    dev = lambda a: torch.from_numpy(a).cuda()
    return dev(theta0), dev(ema0), tuple(dev(g) for g in grads), dev(bad)


def run_path(K, path, n):
    """Three steps of ``path`` on fresh buffers of ``n`` elements -> {tensor name: SHA-256 of its bytes after steps 1, 2, 3}."""
    entry, o = PATHS[path]
    theta0, ema0, grads, bad = problem(n)
    theta, ema = theta0.clone(), ema0.clone()
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    ema_state = torch.full((2,), -1.0, device="cuda")
    guard = torch.zeros(4, dtype=torch.float64, device="cuda")
    ws = K.grad_guard_workspace(n, "cuda")
    sched = torch.tensor(SCHED, dtype=torch.int64, device="cuda") if o.get("sched") else None
    gs, mx = o.get("grad_scale", 1.0), o.get("max_norm", 0.0)
    guarded = entry == "guard" or o.get("guarded", False)
    tensors = {"theta": theta, "m": m, "v": v}
    if entry != "adam":
        tensors["state"] = state
    if entry == "ema":
        tensors.update(ema=ema, ema_state=ema_state)
    if guarded:
        tensors.update(guard=guard, ws_header=ws[:16])
    digests = {k: hashlib.sha256() for k in tensors}
    for step in (1, 2, 3):
        g = bad if o.get("nan") and step == NAN_AT else grads[step - 1]
        if entry == "adam":
            K.adam(theta, g, m, v, step, LR, B1, B2, EPS, gs)
        elif entry == "iter":
            K.adam_iter(theta, g, m, v, state, LR, B1, B2, EPS, gs)
        elif entry == "sched":
            K.adam_sched(theta, g, m, v, state, sched, LR, B1, B2, EPS, gs)
        elif entry == "guard":
            K.adam_guard(theta, g, m, v, state, guard, ws, sched, LR, B1, B2, EPS, gs, mx)
        else:
            K.adam_ema(theta, g, m, v, ema, state, ema_state, EMA_DECAY, sched, LR, B1, B2, EPS, gs,
                       guard if guarded else None, ws if guarded else None, mx)
        for k, t in tensors.items():
            digests[k].update(t.cpu().numpy().tobytes())
    # what the variants are there for did happen (properties of the inputs, not of the fixture)
    if entry != "adam":
        assert state[0].item() == (2 if o.get("nan") else 3), path
    if guarded:
        rec = guard.tolist()
        assert rec[2:] == ([1.0, 2.0] if o.get("nan") else [0.0, 3.0]), (path, rec)
        assert (rec[1] < 1.0) == (mx > 0.0), (path, rec)
    return {k: d.hexdigest() for k, d in digests.items()}


@pytest.fixture(scope="module")
def K():
    import sggan_amd
    import sggan_amd.kernels
    return sggan_amd.kernels


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_covers_every_path_and_size(recorded):
    assert recorded["rocm"] and set(recorded["digests"]) == set(PATHS)
    for path, by_size in recorded["digests"].items():
        assert set(by_size) == {str(n) for n in SIZES}, path


@pytest.mark.parametrize("n", SIZES)
def test_every_path_reproduces_the_recorded_bits(K, recorded, n):
    moved = []
    for path in PATHS:
        got, want = run_path(K, path, n), recorded["digests"][path][str(n)]
        assert set(got) == set(want), (path, n)
        moved += [(path, n, name) for name in got if got[name] != want[name]]
    assert not moved, moved


def test_launches_per_path(K):
    """Each path captured once at n = 5: nodes of the capture, counted with sgg_stream_capture_nodes."""
    from sggan_amd import _abi as A
    n = 5
    theta0, ema0, grads, _ = problem(n)
    theta, ema, g = theta0.clone(), ema0.clone(), grads[0]
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    ema_state = torch.zeros(2, device="cuda")
    guard = torch.zeros(4, dtype=torch.float64, device="cuda")
    ws = K.grad_guard_workspace(n, "cuda")
    sched = torch.tensor(SCHED, dtype=torch.int64, device="cuda")
    bodies = {"adam": lambda: K.adam(theta, g, m, v, 1, LR, B1, B2, EPS),
              "adam_iter": lambda: K.adam_iter(theta, g, m, v, state, LR, B1, B2, EPS),
              "adam_sched": lambda: K.adam_sched(theta, g, m, v, state, sched, LR, B1, B2, EPS),
              "adam_guard": lambda: K.adam_guard(theta, g, m, v, state, guard, ws, None, LR, B1, B2, EPS, 1.0, MAX_NORM),
              "adam_ema plain": lambda: K.adam_ema(theta, g, m, v, ema, state, ema_state, EMA_DECAY, None, LR, B1, B2, EPS),
              "adam_ema guarded": lambda: K.adam_ema(theta, g, m, v, ema, state, ema_state, EMA_DECAY, None, LR, B1, B2, EPS, 1.0,
                                                     guard, ws, MAX_NORM)}
    counts = {}
    for name, body in bodies.items():
        body()                                                   # (once outside: nothing is loaded or allocated inside the capture)
        torch.cuda.synchronize()
        graph, nodes = torch.cuda.CUDAGraph(), C.c_int(0)
        with torch.cuda.graph(graph):
            body()
            A.check(A.lib().sgg_stream_capture_nodes(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(nodes)), "nodes")
        counts[name] = nodes.value
    assert counts == {"adam": 1, "adam_iter": 2, "adam_sched": 2, "adam_guard": 3, "adam_ema plain": 2, "adam_ema guarded": 3}
