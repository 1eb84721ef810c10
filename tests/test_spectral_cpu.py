"""Spectral-norm discriminators (--d_norm spectral), the part that needs no GPU: the float64 oracle checked against
itself, the header and its binding, status codes that are decided before any launch, and the interface."""
import ctypes
import os
import re

import numpy as np
import pytest

from sggan_amd import _abi as A
from tests import spectral_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sgg_spectral_sigma", "sgg_spectral_grad", "sgg_pack_conv_weights_batch_scaled")
QUERIES = ("sgg_spectral_sigma_workspace", "sgg_spectral_grad_workspace")


# ---- oracle self-checks ----------------------------------------------------------------------------------------------------
def _with_singular_values(rng, rows, K, sv):
    a, _ = np.linalg.qr(rng.standard_normal((rows, rows)))
    b, _ = np.linalg.qr(rng.standard_normal((K, K)))
    d = np.zeros((rows, K))
    d[np.arange(len(sv)), np.arange(len(sv))] = sv
    return a @ d @ b.T


def test_thirty_iterations_reach_the_top_singular_value():
    rng = np.random.default_rng(3)
    sv = [3.0, 1.0, 0.5, 0.25, 0.125, 0.1, 0.05, 0.01]
    M = _with_singular_values(rng, 27, 8, sv)
    W = M.reshape(3, 3, 3, 8)
    u = rng.standard_normal(8)
    u /= np.linalg.norm(u)
    for _ in range(30):
        u, v, sigma = S.power_iteration(W, u)
    top = np.linalg.svd(M, compute_uv=False)[0]
    assert abs(top - 3.0) < 1e-12 and abs(sigma - top) < 1e-12
    assert abs(np.linalg.norm(u) - 1) < 1e-14 and abs(np.linalg.norm(v) - 1) < 1e-14
    # without advancing: u keeps its bits and sigma is |M u|
    u2, v2, s2 = S.power_iteration(W, u, advance=False)
    assert u2 is not None and np.array_equal(u2, u) and abs(s2 - np.linalg.norm(M @ u)) < 1e-14


def test_zero_kernel_gives_the_floor():
    u, v, sigma = S.power_iteration(np.zeros((3, 3, 2, 4)), np.ones(4) / 2)
    assert sigma == 1e-12 and np.all(v == 0) and np.all(u == 0) and np.isfinite(1.0 / sigma)


@pytest.mark.parametrize("shape", [(3, 3, 3, 8), (3, 3, 8, 5)])
def test_transform_is_the_gradient_of_the_normalised_kernel_with_u_and_v_fixed(shape):
    rng = np.random.default_rng(11)
    W, Cm = rng.standard_normal(shape), rng.standard_normal(shape)
    u = rng.standard_normal(shape[-1])
    u /= np.linalg.norm(u)
    u, v, sigma = S.power_iteration(W, u)
    sig = lambda w: float(v @ S.mat(w) @ u)
    assert abs(sig(W) - sigma) < 1e-14
    L = lambda w: float((Cm * (w / sig(w))).sum())
    dW = S.grad_transform(Cm, W, u, v, 1.0 / sigma)
    h, fd = 1e-6, np.zeros(shape)
    for idx in np.ndindex(*shape):
        e = np.zeros(shape)
        e[idx] = h
        fd[idx] = (L(W + e) - L(W - e)) / (2 * h)
    assert np.abs(fd - dW).max() < 1e-8 * max(np.abs(dW).max(), 1.0)
    # W / sigma(W) does not change along W, so the gradient has no component along it
    assert abs(float((dW * W).sum())) < 1e-12 * np.linalg.norm(dW) * np.linalg.norm(W)


def test_the_tape_op_carries_the_same_transform():
    from oracle import sggan_oracle as O
    rng = np.random.default_rng(5)
    W, gy = rng.standard_normal((3, 3, 4, 6)), rng.standard_normal((3, 3, 4, 6))
    u0 = rng.standard_normal(6)
    u, v, sigma = S.power_iteration(W, u0 / np.linalg.norm(u0))
    tape, w = O.Tape(), O.Var(W)
    y = S.spectral_scale(tape, w, u, v)
    assert np.allclose(y.v, W / sigma, rtol=1e-15, atol=0)
    tape.backward([(y, gy)])
    assert np.array_equal(w.g, S.grad_transform(gy, W, u, v, 1.0 / sigma))


def test_sign_policy_changes_nothing_where_signs_are_decidable_and_follows_the_images_where_not():
    from oracle import sggan_oracle as O
    rng = np.random.default_rng(9)
    t, w = rng.uniform(0, 1, (1, 12, 12, 3)), (rng.uniform(size=(1, 12, 12, 1)) > 0.4).astype(float)
    x0 = rng.uniform(0, 1, (1, 12, 12, 3))

    def grad(fn):
        tape, x = O.Tape(), O.Var(x0)
        y = fn(tape, x)
        tape.backward([(y, 1.0)])
        return float(y.v), x.g
    pol = S.SignPolicy(1e-4)
    for plain, mine in ((lambda tp, x: O.gradloss(tp, x, t, w), lambda tp, x: S.gradloss(tp, x, t, w, pol, x0 + 1e-9)),
                        (lambda tp, x: O.l1_mean(tp, t, x), lambda tp, x: S.l1_mean(tp, t, x, pol, x0 + 1e-9))):
        (y0, g0), (y1, g1) = grad(plain), grad(mine)
        assert y0 == y1 and np.array_equal(g0, g1)
    assert pol.elements > 0 and pol.disagree_outside == 0
    # an element within the margin takes the images' side; one outside it that disagrees is counted
    pol = S.SignPolicy(1e-4)
    arg, dev = np.array([1e-6, -2e-5, 0.5, -0.5]), np.array([-1e-6, -2e-5, 0.5, 0.5])
    assert np.array_equal(pol.decide(arg, dev), [-1.0, -1.0, 1.0, -1.0])
    assert (pol.ambiguous, pol.overridden, pol.disagree_outside) == (2, 1, 1)


# ---- header and binding ------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sggan.h")).read(), flags=re.S)


def test_entries_are_declared_and_bound_with_matching_types():
    src = _header()
    vp, i, i64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    want = {"sgg_spectral_sigma_workspace": (sz, [i, i, i]),
            "sgg_spectral_sigma": (i, [vp, i, i, i, i, vp, sz, vp]),
            "sgg_spectral_grad_workspace": (sz, [i, i]),
            "sgg_spectral_grad": (i, [vp, i, i, i, vp, sz, vp]),
            "sgg_pack_conv_weights_batch_scaled": (i, [vp, vp, i, i64, i, vp])}
    kinds = {"int": i, "int64_t": i64, "size_t": sz}
    L = A.lib()
    for name in ENTRIES + QUERIES:
        m = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, f"{name} is not declared in include/sggan.h"
        args = [a.strip() for a in m.group(2).split(",")]
        parsed = [vp if "*" in a else kinds[a.split()[0]] for a in args]
        assert (kinds[m.group(1)], parsed) == want[name] == A.SIGNATURES[name], name
        assert getattr(L, name).argtypes == want[name][1]
    # the item struct: six pointers, then rows and K
    m = re.search(r"typedef struct sgg_spectral_item \{(.*?)\} sgg_spectral_item;", src, flags=re.S)
    fields = re.findall(r"(\w+)\s*(?:,\s*(\w+)\s*)?;", m.group(1))
    names = [n for pair in fields for n in pair if n]
    assert names == [f for f, _ in A.SpectralItem._fields_] and ctypes.sizeof(A.SpectralItem) == 56
    assert f"#define SGG_SPECTRAL_BAND {A.SPECTRAL_BAND}" in src and f"#define SGG_SPECTRAL_MAX_K {A.SPECTRAL_MAX_K}" in src


def test_status_is_decided_before_any_launch():
    L = A.lib()
    table = ctypes.create_string_buffer(56)             # host memory: a call that got as far as a launch would not return a status
    t = ctypes.cast(table, ctypes.c_void_p)
    assert L.sgg_spectral_sigma(None, 1, 27, 8, 1, t, 1 << 20, None) == A.EINVAL
    assert L.sgg_spectral_sigma(t, 0, 27, 8, 1, t, 1 << 20, None) == A.EINVAL
    assert L.sgg_spectral_sigma(t, -3, 27, 8, 1, t, 1 << 20, None) == A.EINVAL
    assert L.sgg_spectral_sigma(t, 1, 0, 8, 1, t, 1 << 20, None) == A.EINVAL
    assert L.sgg_spectral_sigma(t, 1, 27, A.SPECTRAL_MAX_K + 1, 1, t, 1 << 30, None) == A.EINVAL
    assert L.sgg_spectral_sigma(t, 1, 27, 8, 1, None, 1 << 20, None) == A.EWORKSPACE
    assert L.sgg_spectral_sigma(t, 1, 27, 8, 1, t, 8, None) == A.EWORKSPACE
    assert L.sgg_spectral_grad(None, 1, 27, 8, t, 1 << 20, None) == A.EINVAL
    assert L.sgg_spectral_grad(t, 0, 27, 8, t, 1 << 20, None) == A.EINVAL
    assert L.sgg_spectral_grad(t, 1, 27, 8, None, 0, None) == A.EWORKSPACE
    assert L.sgg_pack_conv_weights_batch_scaled(None, t, 1, 64, A.SGG_F32, None) == A.EINVAL
    assert L.sgg_pack_conv_weights_batch_scaled(t, None, 1, 64, A.SGG_F32, None) == A.EINVAL
    assert L.sgg_pack_conv_weights_batch_scaled(t, t, 0, 64, A.SGG_F32, None) == A.EINVAL
    # the workspaces: per item t (rows doubles), K + 1 doubles per band, s (K doubles) and 16 fold sums; one double per band per item
    bands = lambda r: (r + A.SPECTRAL_BAND - 1) // A.SPECTRAL_BAND
    assert L.sgg_spectral_sigma_workspace(3, 4608, 512) == 3 * 8 * (4608 + bands(4608) * 513 + 512 + 16)
    assert L.sgg_spectral_sigma_workspace(1, 27, 8) == 8 * (27 + 9 + 8 + 16)
    assert L.sgg_spectral_grad_workspace(8, 4608) == 8 * 8 * bands(4608) and L.sgg_spectral_grad_workspace(0, 5) == 0
    assert L.sgg_spectral_sigma_workspace(1, 27, A.SPECTRAL_MAX_K + 1) == 0


# ---- interface ---------------------------------------------------------------------------------------------------------------
def test_flag_is_absent_unless_given():
    from sggan_amd.main import build_parser, parse_args
    bare = parse_args([])
    assert "d_norm" not in vars(bare)
    a = parse_args(["--d_norm", "spectral"])
    assert a.d_norm == "spectral" and vars(a).keys() - vars(bare).keys() == {"d_norm"}
    assert all(getattr(a, k) == v for k, v in vars(bare).items())
    assert parse_args(["--d_norm", "instance"]).d_norm == "instance"
    with pytest.raises(SystemExit):
        parse_args(["--d_norm", "batch"])
    assert "--d_norm" in build_parser().format_help()


def test_unknown_d_norm_is_refused_before_a_network_is_built():
    import sggan_amd
    from sggan_amd.module import Discriminator, discriminator_param_specs
    assert sggan_amd.default_args().d_norm == "instance" and sggan_amd.default_args(d_norm="spectral").d_norm == "spectral"
    # (the device is refused with another exception type, and later: a ValueError here comes from the option alone)
    with pytest.raises(ValueError, match="d_norm"):
        sggan_amd.sggan(sggan_amd.default_args(d_norm="layer", device="cpu"))
    with pytest.raises(ValueError, match="d_norm"):
        sggan_amd.sggan(d_norm="weight", device="cpu")
    with pytest.raises(ValueError, match="d_norm"):
        Discriminator(norm="batch", device="cpu")
    with pytest.raises(ValueError, match="d_norm"):
        discriminator_param_specs(norm="none")
    with pytest.raises(NotImplementedError):             # a valid value gets as far as the device check
        sggan_amd.sggan(d_norm="spectral", device="cpu")


def test_spectral_specs_are_kernel_and_bias_only():
    from sggan_amd.module import discriminator_param_specs
    sp = discriminator_param_specs(df_dim=8, norm="spectral")
    assert len(sp) == 16 and [n for n, _ in sp] == [f"{l}_{k}" for l in S.LAYERS for k in ("w", "b")]
    assert sp == [(n, tuple(s)) for n, s in S.discriminator_param_shapes(df_dim=8)]
    inst = discriminator_param_specs(df_dim=8)
    assert inst == discriminator_param_specs(df_dim=8, norm="instance") and len(inst) == 28
    assert [e for e in inst if e[0].endswith(("_w", "_b"))] == sp


def test_checkpoint_kind_is_checked_on_host_memory_stores():
    """state_dict / load_state_dict on stores in host memory: an instance model writes no new key; the two kinds refuse each other."""
    import torch
    from sggan_amd.model import sggan
    from sggan_amd.module import ParamStore, discriminator_param_specs, generator_param_specs

    class Net:
        def __init__(self, specs, u=None):
            self.P, self._u = ParamStore(specs, "cpu"), u

        def spectral_state(self):
            return self._u

        def set_spectral_state(self, u=None):
            self._u = torch.zeros(4) if u is None else u.clone()

    def model(kind):
        m = sggan.__new__(sggan)
        m.cycle, m.arch, m.ema_decay, m._ema_notice, m._sn_notice, m.d_norm = False, "resnet", None, False, False, kind
        m.generator = Net(generator_param_specs(gf_dim=8, n_blocks=1))
        m.discriminator = Net(discriminator_param_specs(df_dim=8, norm=kind), torch.arange(4.0) if kind == "spectral" else None)
        return m

    inst, spec = model("instance"), model("spectral")
    assert set(inst.state_dict()["D"]) == {"flat", "m", "v", "t"}
    sd = spec.state_dict()
    assert set(sd["D"]) == {"flat", "m", "v", "t", "d_norm", "u"} and sd["D"]["d_norm"] == "spectral"
    with pytest.raises(ValueError, match="spectral-norm.*instance-norm"):
        inst.load_state_dict(sd)
    with pytest.raises(ValueError, match="instance-norm.*spectral-norm"):
        spec.load_state_dict(inst.state_dict())
    other = model("spectral")
    other.load_state_dict(sd)
    assert torch.equal(other.discriminator.spectral_state(), torch.arange(4.0))
    del sd["D"]["u"]                                      # a spectral checkpoint without vectors: the seeded start, one notice
    other.load_state_dict(sd)
    assert other._sn_notice and torch.equal(other.discriminator.spectral_state(), torch.zeros(4))
