"""CPU-side checks of the guarded optimizer step (--clip_grad_norm / --skip_nonfinite): the host statement
of the rule (kernels.guarded_update) against an independent elementwise form, the C ABI of the three new entry points, the
build resources of the three new kernels and the flags."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from sggan_amd import _abi as A
from tests.kernel_resources import kernel_resource_usage, the_kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, B1, B2, EPS = 2e-4, 0.5, 0.999, 1e-7


def _loop_form(theta, g, m, v, iterations, lr, b1, b2, eps, grad_scale, max_norm, sched=None):
    """The rule written a second time, one element after the other in Python floats (math, no NumPy arithmetic): f32 launch
    arguments, float64 everything else."""
    f = lambda x: float(np.float32(x))
    n = len(g)
    skip = any(math.isnan(x) or math.isinf(x) for x in g)
    ss = 0.0
    for x in g:
        ss += x * x
    norm = math.sqrt(ss) * f(grad_scale) if not math.isnan(ss) else float("nan")
    clip = 1.0
    if not skip and f(max_norm) > 0 and not norm <= f(max_norm):
        clip = f(f(max_norm) / norm)
    if skip:
        return list(theta), list(m), list(v), iterations, norm, clip, True
    t = iterations + 1
    lr_e = f(lr)
    if sched is not None:
        spe, step, epochs = max(sched[0], 1), sched[1], sched[2]
        e = iterations // spe
        if not (epochs <= step or e < step):
            lr_e = f(f(lr) * max(epochs - e, 0) / (epochs - step))
    lr_t = lr_e * math.sqrt(1.0 - f(b2) ** t) / (1.0 - f(b1) ** t)
    factor = f(np.float32(grad_scale) * np.float32(clip))
    th2, m2, v2 = [], [], []
    for i in range(n):
        gi = g[i] * factor
        mi = f(b1) * m[i] + (1.0 - f(b1)) * gi
        vi = f(b2) * v[i] + (1.0 - f(b2)) * gi * gi
        th2.append(theta[i] - lr_t * mi / (math.sqrt(vi) + f(eps)))
        m2.append(mi); v2.append(vi)
    return th2, m2, v2, t, norm, clip, False


def _case(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n), rng.standard_normal(n) * scale, rng.standard_normal(n) * 0.1, rng.random(n) * 0.01)


@pytest.mark.parametrize("case", ["finite_off", "finite_under", "clipped", "clipped_dp", "clipped_sched", "nan", "inf", "overflow"])
def test_guarded_update_against_the_loop_form(case):
    """kernels.guarded_update == the elementwise loop form to 1e-12 (relative to 1 + |value|), for a finite gradient with the
    clip off, one under the bound, clipped ones (plain, with grad_scale = 1/2, with a decaying rate), a NaN, a -Inf, and a finite
    gradient whose f32 sum of squares would overflow."""
    from sggan_amd.kernels import guarded_update
    n = 37
    theta, g, m, v = _case(n, 11, 1e20 if case == "overflow" else 1.0)
    kw = dict(lr=LR, beta1=B1, beta2=B2, eps=EPS, grad_scale=1.0, max_norm=0.0)
    sched = None
    norm0 = float(np.sqrt(np.sum(g * g)))
    if case == "finite_under":
        kw["max_norm"] = 2.0 * norm0
    elif case in ("clipped", "overflow"):
        kw["max_norm"] = 0.5 * norm0 if case == "clipped" else 1.0
    elif case == "clipped_dp":
        kw.update(grad_scale=0.5, max_norm=0.25 * norm0)
    elif case == "clipped_sched":
        kw["max_norm"], sched = 0.5 * norm0, (2, 1, 4)
    elif case == "nan":
        g[5] = np.nan
    elif case == "inf":
        g[n - 1] = -np.inf
    it = 5
    th1, m1, v1, t1, info = guarded_update(theta, g, m, v, it, sched=sched, **kw)
    th2, m2, v2, t2, norm2, clip2, skip2 = _loop_form(list(theta), list(g), list(m), list(v), it, kw["lr"], kw["beta1"], kw["beta2"],
                                                      kw["eps"], kw["grad_scale"], kw["max_norm"], sched)
    assert t1 == t2 and info["skip"] == skip2
    for a, b in ((th1, th2), (m1, m2), (v1, v2)):
        a, b = np.asarray(a), np.asarray(b)
        assert np.all(np.abs(a - b) <= 1e-12 * (1.0 + np.abs(b)))
    if case in ("nan", "inf"):
        assert info["skip"] and t1 == it and not np.isfinite(info["norm"]) and info["clip"] == 1.0
        assert np.array_equal(th1, theta) and np.array_equal(m1, m) and np.array_equal(v1, v)
    else:
        assert not info["skip"] and t1 == it + 1
        assert abs(info["norm"] - norm2) <= 1e-12 * norm2 and info["clip"] == clip2
        assert (info["clip"] < 1.0) == (case.startswith("clipped") or case == "overflow")
        if case == "clipped_dp":                           # max_norm means the same at any world size: the SCALED norm is clipped
            assert abs(info["norm"] - 0.5 * norm0) <= 1e-12 * norm0 and abs(info["clip"] - 0.5) < 1e-6
        if case == "overflow":
            assert np.isfinite(info["norm"]) and info["norm"] > 1e20 and float(np.float32(norm0)) ** 2 > float(np.finfo(np.float32).max) and np.all(np.isfinite(th1))


def test_guard_entry_points_are_exported_bound_and_validate_on_the_host():
    """The three symbols are declared with the issue's signatures and bound with matching ctypes; the workspace is 16 bytes
    plus 16 per chunk of GRAD_GUARD_CHUNK elements; a short workspace returns SGG_EWORKSPACE and null pointers / n <= 0 return
    SGG_EINVAL -- all before any launch, so no GPU is needed (the buffers are host memory that is never dereferenced)."""
    from sggan_amd import kernels as K
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sggan.h")).read(), flags=re.S)
    def params(name):
        decl = re.search(r"\b%s\((.*?)\);" % name, src, flags=re.S)
        assert decl, name + " not declared"
        return [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params("size_t sgg_grad_guard_workspace") == ["int64_t n"]
    assert params("int sgg_grad_sumsq") == ["const float* g", "int64_t n", "void* ws", "size_t ws_bytes", "void* stream"]
    assert params("int sgg_adam_guard") == [
        "float* theta", "const float* g", "float* m", "float* v", "int64_t n", "int64_t* state", "const int64_t* sched", "float lr",
        "float beta1", "float beta2", "float eps", "float grad_scale", "float max_norm", "double* guard", "void* ws", "size_t ws_bytes",
        "void* stream"]
    vp, f, i64, sz = C.c_void_p, C.c_float, C.c_int64, C.c_size_t
    assert A.SIGNATURES["sgg_grad_guard_workspace"] == (sz, [i64])
    assert A.SIGNATURES["sgg_grad_sumsq"] == (C.c_int, [vp, i64, vp, sz, vp])
    assert A.SIGNATURES["sgg_adam_guard"] == (C.c_int, [vp, vp, vp, vp, i64, vp, vp, f, f, f, f, f, f, vp, vp, sz, vp])
    L = A.lib()
    chunk = K.GRAD_GUARD_CHUNK
    assert chunk % 1024 == 0
    for n in (1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 7, 22 * 10 ** 6, (1 << 31) + 5):
        assert L.sgg_grad_guard_workspace(n) == 16 + 16 * ((n + chunk - 1) // chunk), n
    assert L.sgg_grad_guard_workspace(0) == 0 and L.sgg_grad_guard_workspace(-4) == 0

    raw = (C.c_char * 256)()
    base = (C.addressof(raw) + 15) & ~15                    # a 16-byte aligned host address
    p, odd = C.c_void_p(base), C.c_void_p(base + 4)
    n = 2 * chunk + 7
    need = L.sgg_grad_guard_workspace(n)
    hp = (LR, B1, B2, EPS, 1.0, 1.0)
    assert L.sgg_grad_sumsq(p, n, p, need - 1, None) == A.EWORKSPACE
    assert L.sgg_grad_sumsq(p, n, p, 0, None) == A.EWORKSPACE
    assert L.sgg_adam_guard(p, p, p, p, n, p, None, *hp, p, p, need - 1, None) == A.EWORKSPACE
    assert L.sgg_adam_guard(p, p, p, p, n, p, p, *hp, p, p, 16, None) == A.EWORKSPACE
    assert L.sgg_grad_sumsq(None, n, p, need, None) == A.EINVAL
    assert L.sgg_grad_sumsq(p, n, None, need, None) == A.EINVAL
    assert L.sgg_grad_sumsq(p, 0, p, need, None) == A.EINVAL and L.sgg_grad_sumsq(p, -1, p, need, None) == A.EINVAL
    assert L.sgg_grad_sumsq(odd, n, p, need, None) == A.EINVAL and L.sgg_grad_sumsq(p, n, odd, need, None) == A.EINVAL   # alignment
    for hole in range(8):                                   # theta, g, m, v, state, guard, ws missing in turn; then n <= 0
        a = [p, p, p, p, p, p, p]
        if hole < 7:
            a[hole] = None
        nn = n if hole < 7 else 0
        assert L.sgg_adam_guard(a[0], a[1], a[2], a[3], nn, a[4], None, *hp, a[5], a[6], need, None) == A.EINVAL, hole


def test_guard_kernels_do_not_spill_and_use_no_scratch(tmp_path):
    """csrc/adam.hip recompiled with -Rpass-analysis=kernel-resource-usage (tests/kernel_resources.py): the three kernels of a
    guarded update are in the build with zero VGPR / SGPR spills and no scratch, at full occupancy (8 waves per SIMD: the
    sum-of-squares pass hides HBM latency with resident blocks), and the two reductions hold their 256 doubles + 256 flags of LDS."""
    usage = kernel_resource_usage("adam.hip", tmp_path)
    for frag, lds in (("gradsq_partial_kernel", 3072), ("adam_prep_kernel", 3072), ("adam_kernel", 0)):
        u = the_kernel(usage, frag)
        assert {k: u[k] for k in ("vspill", "sspill", "scratch", "occ", "lds")} == {"vspill": 0, "sspill": 0, "scratch": 0, "occ": 8, "lds": lds}, (frag, u)


def test_guard_flags_and_default_arguments():
    """--clip_grad_norm FLOAT and --skip_nonfinite parse; without them the namespace is the one it was before they existed (they
    are absent, and sggan reads 0 / off), so a run without them is configured exactly as before."""
    from sggan_amd.main import build_parser, parse_args
    from sggan_amd.model import default_args
    a = parse_args(["--clip_grad_norm", "2.5", "--skip_nonfinite"])
    assert a.clip_grad_norm == 2.5 and a.skip_nonfinite is True
    assert parse_args(["--clip_grad_norm", "1"]).clip_grad_norm == 1.0
    plain = vars(parse_args([]))
    assert "clip_grad_norm" not in plain and "skip_nonfinite" not in plain
    assert not hasattr(parse_args(["--skip_nonfinite"]), "clip_grad_norm")
    with pytest.raises(SystemExit):
        parse_args(["--clip_grad_norm", "big"])
    text = " ".join(build_parser().format_help().split())
    for word in ("--clip_grad_norm", "--skip_nonfinite", "default 0 = off", "global L2 norm", "NaN or Inf"):
        assert word in text, word
    d = default_args()
    assert d.clip_grad_norm == 0.0 and d.skip_nonfinite is False
    assert default_args(clip_grad_norm=3.0, skip_nonfinite=True).clip_grad_norm == 3.0


def test_optimizer_options_are_off_by_default():
    """module.Adam: clip_norm None / <= 0 and skip_nonfinite False select the unguarded calls (ParamStore.adam_step makes no new
    launch and allocates no guard record)."""
    from sggan_amd.module import Adam, ParamStore, discriminator_param_specs

    class _Net:
        P = ParamStore(discriminator_param_specs(df_dim=8), "cpu")
    o = Adam(_Net())
    assert o.clip_norm is None and o.skip_nonfinite is False and _Net.P._guard is None and _Net.P._guard_ws is None
    assert Adam(_Net(), clip_norm=0.0).clip_norm is None and Adam(_Net(), clip_norm=-1).clip_norm is None
    o = Adam(_Net(), clip_norm=2, skip_nonfinite=True)
    assert o.clip_norm == 2.0 and o.skip_nonfinite is True
