"""The small kernels of csrc/misc.hip -- bias gradient, L1 / BCE / LSGAN / Sobel losses, activations, add, channel pad / unpad,
argmax-u8 labels, confusion histogram, segmentation-edge indicator, and Adam (csrc/adam.hip) -- against tests/small_kernels_oracle.py (float64,
written from include/sggan.h) at the shapes where their chunking, grid-stride loops and vector tails change path.

Exact wherever it can be had: inputs k/8, weights in {0, 0.5, 1} and power-of-two scalar factors make every float32 partial
sum and every gradient value exact (tests/test_small_kernels_oracle_cpu.py proves the premise for each case used here), so
sums and gradients are compared for EQUALITY and one dropped or doubled element at any size fails.  Transcendental and
random-data variants use the tolerances of tests/test_gpu_ops.py: 1e-4 of the tensor's scale (f32), 2e-2 (bf16),
1e-6 * max(1, |loss|) for the BCE / LSGAN scalars.  Outputs are pre-filled with NaN (integers: a sentinel); nothing of it
may survive inside the logical extent of a non-accumulating call."""
import numpy as np
import pytest
import torch

from tests import small_kernels_oracle as S

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
NAMES = ["f32", "bf16"]
ACTS = {"none": 0, "relu": 1, "lrelu": 2, "tanh": 3}


@pytest.fixture(scope="module")
def K():
    from sggan_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def A():
    from sggan_amd import _abi
    return _abi


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to("cuda").to(dtype)


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def nans(shape, dtype=torch.float32):
    return torch.full(tuple(shape) if not isinstance(shape, int) else (shape,), float("nan"), dtype=dtype, device="cuda")


def stored(x, dtype):
    """float64 values of x after the f32 evaluation and the RNE store to `dtype` (what a kernel writes for an exact f32 result x)."""
    return torch.as_tensor(np.asarray(x, np.float64).astype(np.float32)).to(dtype).float().numpy().astype(np.float64)


def same(got, exp, what=""):
    """Equality of values with no NaN on either side (+0 == -0)."""
    g, e = host(got) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64), np.asarray(exp, np.float64)
    assert g.shape == e.shape, (what, g.shape, e.shape)
    assert not np.isnan(g).any(), f"{what}: {int(np.isnan(g).sum())} unwritten (NaN) elements"
    bad = g != e
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}: got {g[bad][0]!r}, expected {e[bad][0]!r}"


def close(got, exp, dtype, what="", scale=None):
    g, e = host(got) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64), np.asarray(exp, np.float64)
    assert g.shape == e.shape, (what, g.shape, e.shape)
    assert not np.isnan(g).any(), f"{what}: unwritten (NaN) elements"
    s = scale if scale is not None else max(np.abs(e).max(), 1e-6)
    tol = 1e-4 if dtype == torch.float32 else 2e-2
    err = np.abs(g - e).max() / s
    print(f"{what}: max err {err:.3e} of scale {s:.3e} (tol {tol})")
    assert err < tol, f"{what}: max err {err:.3e} of scale {s:.3e} (tol {tol})"


def f32_add(a, b):
    """One float32 addition (the documented `*loss += l`)."""
    return np.float64(np.float32(np.float32(a) + np.float32(b)))


# ---------------------------------------------------------------------------- bias gradient
def bias_grad_abi(K, A, dy, db, C_real, accumulate=False):
    """sgg_bias_grad with C_real given (K.bias_grad takes it from db.numel()) and a workspace of exactly the queried size."""
    C = dy.shape[-1]
    P = dy.numel() // C
    ws = nans(int(A.lib().sgg_bias_grad_workspace(P, C)) // 4)
    A.check(A.lib().sgg_bias_grad(K._p(dy), K._p(db), P, C, C_real, int(accumulate), K.dt(dy), K._p(ws), ws.numel() * 4, K._s()), "bias_grad")


@pytest.mark.parametrize("name,C", [(n, C) for n in NAMES for C in S.BIAS_C[n]], ids=lambda v: str(v))
def test_bias_grad_exact_at_chunk_edges(K, name, C):
    """C: one vector lane (8), lanes that do not divide 256 (bf16 40: 5, f32 24: 6), several lanes, more than 256 lanes (a second
    pass over the channel vectors); P: one row, one row short of a chunk, a chunk, a chunk + 1, ragged three chunks."""
    for P in S.BIAS_P:
        dy = S.bias_case(C, P)
        db = nans(C)
        K.bias_grad(dev(dy, DT[name]), db)
        same(db, S.colsum(dy, C), f"db C={C} P={P}")


@pytest.mark.parametrize("name", NAMES)
def test_bias_grad_more_than_256_chunks_creal_accumulate(K, A, name):
    dy = S.bias_case(8, S.BIAS_P_BIG)
    t = dev(dy, DT[name])
    db = nans(8)
    K.bias_grad(t, db)
    same(db, S.colsum(dy, 8), "db, 258 chunks")
    # C_real < C: a longer buffer keeps its entries from C_real on
    dy = S.bias_case(40, 1025)
    t = dev(dy, DT[name])
    db = torch.cat([nans(34), torch.full((6,), 777.0, device="cuda")])
    bias_grad_abi(K, A, t, db, 34)
    same(db, np.concatenate([S.colsum(dy, 34), np.full(6, 777.0)]), "db, C_real 34 of 40")
    # accumulate onto integer contents
    base = np.arange(40.0) - 20
    db = dev(base)
    bias_grad_abi(K, A, t, db, 34, accumulate=True)
    same(db, base + np.concatenate([S.colsum(dy, 34), np.zeros(6)]), "db accumulated")
    db = dev(base)
    K.bias_grad(t, db, accumulate=True)
    same(db, base + S.colsum(dy, 40), "db accumulated, all channels")


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("C,P", [(40, 1025), (520, 3000)])
def test_bias_grad_group2_against_the_oracle(K, name, C, P):
    """Two networks' tensors back to back: each half against ITS column sums (the group2-vs-single check of test_gpu_ops.py
    passes when both are wrong)."""
    d0, d1 = S.bias_case(C, P, seed=0), S.bias_case(C, P, seed=1)
    t = dev(np.stack([d0, d1]), DT[name])
    db, db2 = nans(C), nans(C)
    K.bias_grad_group2(t, db, db2)
    same(db, S.colsum(d0, C), "db"); same(db2, S.colsum(d1, C), "db2")
    base = np.arange(float(C)) % 17 - 8
    db, db2 = dev(base), dev(-base)
    K.bias_grad_group2(t, db, db2, accumulate=True)
    same(db, base + S.colsum(d0, C), "db accumulated"); same(db2, S.colsum(d1, C) - base, "db2 accumulated")


# ---------------------------------------------------------------------------- L1 loss
def l1_check(K, name, P, Cr, Cp, flags=False):
    dtype = DT[name]
    a, b, weight, factor = S.l1_case(P, Cr, Cp)
    ta, tb = dev(a, dtype), dev(b, dtype)
    exp_loss = np.float64(np.float32(S.l1_sum(a, b, Cr) * factor))
    tag = f"l1 P={P} ({Cr},{Cp})"
    loss, db = nans(1), nans((P, Cp), dtype)
    K.l1_loss(ta, tb, Cr, loss, db, weight=weight)
    same(loss, [exp_loss], tag + " loss")
    ref_loss, ref_db = S.l1_loss(a, b, Cr, weight)
    assert ref_loss == exp_loss
    same(db, ref_db, tag + " db")                       # +-factor, 0 at ties and in padded channels
    assert not host(db)[:, Cr:].any()
    if not flags:
        return
    loss = nans(1)
    K.l1_loss(ta, tb, Cr, loss, None, weight=weight)
    same(loss, [exp_loss], tag + " loss, db=None")
    loss, db = nans(1), nans((P, Cp), dtype)
    K.l1_loss(ta, tb, Cr, loss, db, weight=weight, gscale=0.5)
    same(loss, [exp_loss], tag + " loss, gscale"); same(db, 0.5 * ref_db, tag + " db, gscale")
    old = np.random.default_rng(P).integers(-8, 9, (P, Cp)) * factor
    for acc, accg in ((True, False), (False, True), (True, True)):
        loss, db = dev([3.0]), dev(old, dtype)
        K.l1_loss(ta, tb, Cr, loss, db, weight=weight, accumulate=acc, accumulate_grad=accg)
        same(loss, [f32_add(3.0, exp_loss) if acc else exp_loss], tag + f" loss acc={acc},{accg}")
        same(db, old + ref_db if accg else ref_db, tag + f" db acc={acc},{accg}")


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("Cr,Cp", S.L1_SHAPES)
def test_l1_loss_exact_at_chunk_edges_and_flags(K, name, Cr, Cp):
    """One vector, one short of a chunk of 2048 vectors, a chunk, a chunk + 1, ragged three chunks (the smallest pixel counts with
    at least that many vectors); (10, 16): C_real ends inside a vector.  Flags at the ragged sizes."""
    for nvec in S.L1_NVEC:
        l1_check(K, name, S.l1_pixels(nvec, Cp, name), Cr, Cp, flags=nvec in (1, 2049, 5000))


def test_l1_loss_more_than_256_chunks(K):
    l1_check(K, "f32", S.L1_P_BIG, 3, 8)


# ---------------------------------------------------------------------------- BCE with logits / LSGAN criterion
def logits_case(n, seed):
    x = (np.random.default_rng([21, n, seed]).standard_normal(n) * 3).astype(np.float32).astype(np.float64)
    if n >= 255:
        x[[3, 100, 200, n - 1]] = (30.0, -30.0, 100.0, -100.0)
    return x


@pytest.mark.parametrize("op", ["bce_logits", "mse_const"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_scalar_losses_tails_flags_and_extreme_logits(K, op, n):
    fn, ref = getattr(K, op), getattr(S, op)
    xs = [logits_case(n, 0)] if n > 1 else [np.array([v]) for v in (0.75, 30.0, -30.0, 100.0, -100.0)]
    for x in xs:
        tx = dev(x)
        for label in (0.0, 1.0, 0.9):
            tag = f"{op} n={n} label={label} x0={x[0]}"
            exp_loss, exp_dx = ref(x, label, weight=0.5, gscale=0.25)
            loss, dx = nans(1), nans(n)
            fn(tx, label, loss, dx, weight=0.5, gscale=0.25)
            got = float(loss.item())
            print(f"{tag}: loss {got!r} oracle {exp_loss!r} err {abs(got - exp_loss):.3e}")
            assert np.isfinite(got) and abs(got - exp_loss) < 1e-6 * max(1.0, abs(exp_loss)), tag
            close(dx, exp_dx, torch.float32, tag + " dx")
            assert np.isfinite(host(dx)).all()
            # dx = None with a loss; loss = None with a dx; both accumulate bits
            loss2 = nans(1)
            fn(tx, label, loss2, None, weight=0.5, gscale=0.25)
            assert torch.equal(loss2, loss), tag + " dx=None"
            dx2 = nans(n)
            fn(tx, label, None, dx2, weight=0.5, gscale=0.25)
            assert torch.equal(dx2, dx), tag + " loss=None"
            old = (np.linspace(-1.0, 1.0, n) * np.abs(exp_dx).max()).astype(np.float32).astype(np.float64)   # of the gradient's size
            loss3, dx3 = dev([2.0]), dev(old)
            fn(tx, label, loss3, dx3, weight=0.5, gscale=0.25, accumulate_grad=True)
            assert torch.equal(loss3, loss), tag + " accumulate_grad leaves the loss bit alone"
            # scale: that of the two addends (at n = 1 they cancel to 0; an f32 sum errs by 2^-24 of its operands, not of the result)
            close(dx3, old + exp_dx, torch.float32, tag + " dx accumulated", scale=max(np.abs(exp_dx).max(), 1e-6))
            loss4, dx4 = dev([2.0]), nans(n)
            fn(tx, label, loss4, dx4, weight=0.5, gscale=0.25, accumulate_loss=True)
            assert abs(float(loss4.item()) - (2.0 + exp_loss)) < 1e-6 * max(1.0, abs(2.0 + exp_loss)), tag + " loss accumulated"
            assert torch.equal(dx4, dx), tag + " accumulate_loss leaves the gradient bit alone"


# ---------------------------------------------------------------------------- Sobel gradient loss
def gradloss_check(K, name, dims, Cr, Cp, flags=False):
    dtype = DT[name]
    a, b, w, lam, factor = S.gradloss_case(*dims, Cr, Cp)
    ta, tb, tw = dev(a, dtype), dev(b, dtype), dev(w)
    ref_loss, ref_din = S.gradloss(a, b, w, Cr, lam)
    exp_loss = np.float64(np.float32(ref_loss))
    assert exp_loss == ref_loss
    tag = f"gradloss {dims} ({Cr},{Cp})"
    loss, din = nans(1), nans(a.shape, dtype)
    K.gradloss(ta, tb, tw, Cr, loss, din, lam=lam)
    same(loss, [exp_loss], tag + " loss")
    same(din, ref_din, tag + " din")
    assert not host(din)[..., Cr:].any()
    if not flags:
        return
    loss = nans(1)
    K.gradloss(ta, tb, tw, Cr, loss, None, lam=lam)
    same(loss, [exp_loss], tag + " loss, dx=None")
    loss, din = nans(1), nans(a.shape, dtype)
    K.gradloss(ta, tb, tw, Cr, loss, din, lam=lam, gscale=0.5)
    same(loss, [exp_loss], tag + " loss, gscale"); same(din, 0.5 * ref_din, tag + " din, gscale")
    old = np.random.default_rng(7).integers(-8, 9, a.shape) * factor
    for acc, accg in ((True, False), (False, True), (True, True)):
        loss, din = dev([3.0]), dev(old, dtype)
        K.gradloss(ta, tb, tw, Cr, loss, din, lam=lam, accumulate_loss=acc, accumulate_grad=accg)
        same(loss, [f32_add(3.0, exp_loss) if acc else exp_loss], tag + f" loss acc={acc},{accg}")
        same(din, old + ref_din if accg else ref_din, tag + f" din acc={acc},{accg}")


GL_CASES = [(n, s) for n in NAMES for s in S.GL_VEC_SHAPES + S.GL_SCALAR_SHAPES if not (n == "bf16" and s[1] % 8)]


@pytest.mark.parametrize("name,shape", GL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_gradloss_exact_on_both_paths(K, name, shape):
    """C_real <= 4 with 8 | Cpad takes the one-thread-per-pixel kernels, (3, 4) and (5, 8) the per-element ones.  Single pixel,
    single row, single column, three different images of 2 x 5 (a neighbour read across an image border shows), 2 x 16 x 24."""
    for dims in S.GL_DIMS:
        gradloss_check(K, name, dims, *shape, flags=dims in ((1, 1, 7), (3, 2, 5)))


@pytest.mark.parametrize("name,shape", [("f32", (3, 8)), ("bf16", (3, 8)), ("f32", (5, 8))], ids=lambda v: str(v).replace(" ", ""))
def test_gradloss_grid_stride(K, name, shape):
    """513 x 512 pixels: more than 1024 blocks x 256 threads, so the first 512 threads take a second pixel."""
    gradloss_check(K, name, S.GL_DIMS_BIG, *shape)


@pytest.mark.parametrize("dims", [(3, 2, 5), (2, 16, 24), S.GL_DIMS_BIG], ids=str)
@pytest.mark.parametrize("data", ["eighths", "normal"])
def test_gradloss_vector_and_scalar_paths_give_the_same_bits(K, dims, data):
    """csrc/misc.hip: "Same pixel -> thread assignment and the same summation order per pixel as the scalar kernels: bit-identical
    results".  The same data as (N,H,W,8) through the vector kernels and as its first 4 channels, contiguous, through the scalar
    ones (Cpad = 4, f32)."""
    rng = np.random.default_rng(31)
    if data == "eighths":
        a, b, w, lam, _ = S.gradloss_case(*dims, 3, 8)
    else:
        a, b = rng.standard_normal(dims + (8,)), rng.uniform(0, 1, dims + (8,))
        w, lam = rng.uniform(0, 1, dims), 5.0
    ta, tb, tw = dev(a), dev(b), dev(w)
    ta4, tb4 = ta[..., :4].contiguous(), tb[..., :4].contiguous()
    for gscale, accg in ((0.5, True), (1.0, False)):
        lv, ls = nans(1), nans(1)
        dv, ds = (torch.ones_like(ta), torch.ones_like(ta4)) if accg else (nans(ta.shape), nans(ta4.shape))
        K.gradloss(ta, tb, tw, 3, lv, dv, lam=lam, gscale=gscale, accumulate_grad=accg)
        K.gradloss(ta4, tb4, tw, 3, ls, ds, lam=lam, gscale=gscale, accumulate_grad=accg)
        assert not torch.isnan(lv).any() and torch.equal(lv.view(torch.int32), ls.view(torch.int32)), (float(lv), float(ls))
        assert not torch.isnan(dv[..., :3]).any()
        assert torch.equal(dv[..., :3].contiguous().view(torch.int32), ds[..., :3].contiguous().view(torch.int32))
    if data == "normal":                                   # and both are the operation: float64 oracle on the same f32 data
        ref_loss, ref_din = S.gradloss(host(ta4), host(tb4), host(tw), 3, lam)
        assert abs(float(ls) - ref_loss) < 1e-4 * abs(ref_loss)
        close(ds, ref_din, torch.float32, "din, scalar path")


@pytest.mark.parametrize("name", NAMES)
def test_gradloss_scalar_path_random_data(K, name):
    """The per-element kernels (C_real = 5) on data that is not dyadic, at the tolerances of test_gpu_ops.py."""
    rng = np.random.default_rng(32)
    dims, Cr, Cp = (2, 9, 11), 5, 8
    ta, tb = dev(np.tanh(rng.standard_normal(dims + (Cp,))), DT[name]), dev(rng.uniform(0, 1, dims + (Cp,)), DT[name])
    w = (rng.uniform(size=dims) > 0.4) * 1.0
    ref_loss, ref_din = S.gradloss(host(ta), host(tb), w, Cr, 5.0)
    loss, din = nans(1), nans(ta.shape, DT[name])
    K.gradloss(ta, tb, dev(w), Cr, loss, din, lam=5.0)
    rel = abs(float(loss) - ref_loss) / abs(ref_loss)
    print(f"gradloss scalar path {name}: loss rel err {rel:.3e}")
    assert rel < (1e-4 if name == "f32" else 2e-2)
    close(din, ref_din, DT[name], "din")
    assert not host(din)[..., Cr:].any()


# ---------------------------------------------------------------------------- activations / add
def act_abi(K, A, fn, *args):
    return getattr(A.lib(), fn)(*args, K._s())


def act_expected(op, act, leak, x, y, dy, dtype):
    """(expected, exact): relu / lrelu / none are one exact product or a copy -- float64, then the f32 evaluation and the RNE
    store; tanh is compared at the tolerance."""
    e = S.act_fwd(x, act, leak) if op == "fwd" else S.act_bwd(dy, y, act, leak)
    return (stored(e, dtype), True) if act != "tanh" else (e, False)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("act,leak", [("none", 0.0), ("relu", 0.0), ("lrelu", 0.2), ("lrelu", 0.3), ("tanh", 0.0)])
def test_act_fwd_bwd_random_dy_zeros_and_one_vector(K, A, name, act, leak):
    dtype = DT[name]
    vec = S.VEC[name]
    rng = np.random.default_rng(41)
    for nvec in (1, 3, 259):
        n = nvec * vec
        x = rng.standard_normal(n) * 2
        x[:3] = (0.0, -0.0, -1.5)
        tx = dev(x, dtype)
        xq = host(tx)
        ty = nans(n, dtype)
        A.check(act_abi(K, A, "sgg_act_fwd", K._p(tx), K._p(ty), n, ACTS[act], leak, K.dt(tx)), "act_fwd")
        exp, exact = act_expected("fwd", act, leak, xq, None, None, dtype)
        (same if exact else lambda g, e, w: close(g, e, dtype, w))(ty, exp, f"{act} fwd n={n}")
        tdy = dev(rng.standard_normal(n), dtype)
        tdx = nans(n, dtype)
        A.check(act_abi(K, A, "sgg_act_bwd", K._p(tdy), K._p(ty), K._p(tdx), n, ACTS[act], leak, K.dt(tx)), "act_bwd")
        exp, exact = act_expected("bwd", act, leak, None, host(ty), host(tdy), dtype)
        (same if exact else lambda g, e, w: close(g, e, dtype, w))(tdx, exp, f"{act} bwd n={n}")
        assert torch.equal(K.act_fwd(tx, ACTS[act], leak), ty) and torch.equal(K.act_bwd(tdy, ty, ACTS[act], leak), tdx)


@pytest.mark.parametrize("name", NAMES)
def test_eltwise_grid_stride_add_and_argument_check(K, A, name):
    """4096 x 256 + 3 vectors: every thread of the capped grid takes a second vector, three of them a third."""
    dtype = DT[name]
    vec = S.VEC[name]
    n = (4096 * 256 + 3) * vec
    gen = torch.Generator().manual_seed(5)
    ca, cb = torch.randn(n, generator=gen).to(dtype), torch.randn(n, generator=gen).to(dtype)
    ta, tb = ca.cuda(), cb.cuda()
    out = nans(n, dtype)
    A.check(act_abi(K, A, "sgg_add", K._p(ta), K._p(tb), K._p(out), n, K.dt(ta)), "add")
    assert torch.equal(out.cpu(), ca + cb), "add: exact in f32, one RNE rounding in bf16"
    assert torch.equal(K.add(ta, tb), out)
    y = nans(n, dtype)
    A.check(act_abi(K, A, "sgg_act_fwd", K._p(ta), K._p(y), n, ACTS["lrelu"], 0.2, K.dt(ta)), "act_fwd")
    same(y, stored(S.act_fwd(host(ta), "lrelu", 0.2), dtype), "lrelu fwd")
    dx = nans(n, dtype)
    A.check(act_abi(K, A, "sgg_act_bwd", K._p(tb), K._p(y), K._p(dx), n, ACTS["lrelu"], 0.2, K.dt(ta)), "act_bwd")
    same(dx, stored(S.act_bwd(host(tb), host(y), "lrelu", 0.2), dtype), "lrelu bwd")
    # n that is no multiple of the vector: rejected before any launch
    bad = nans(vec, dtype)
    for fn, args in (("sgg_act_fwd", (K._p(ta), K._p(bad), vec - 2, 1, 0.0)), ("sgg_act_bwd", (K._p(ta), K._p(tb), K._p(bad), vec - 2, 1, 0.0)),
                     ("sgg_add", (K._p(ta), K._p(tb), K._p(bad), vec - 2))):
        assert act_abi(K, A, fn, *args, K.dt(ta)) == A.EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(bad).all()


# ---------------------------------------------------------------------------- channel pad / unpad
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("Cs,Cd", [(3, 8), (34, 40), (8, 8)])
def test_pad_unpad_channels(K, A, name, Cs, Cd):
    dtype = DT[name]
    gen = torch.Generator().manual_seed(6)
    for P in (1, 257) + ((131075,) if (Cs, Cd) == (3, 8) else ()):            # 131075 * 8 > 4096 * 256: the grid-stride loop
        src = torch.randn((P, Cs), generator=gen)
        exp = torch.zeros((P, Cd), dtype=dtype)
        exp[:, :Cs] = src.to(dtype)                                            # f32: the bits; bf16: torch's RNE cast
        out = nans((P, Cd), dtype)
        K.pad_channels(src.cuda(), Cd, dtype, out=out)
        assert not torch.isnan(out).any() and torch.equal(out.cpu(), exp), f"pad P={P}"
        assert not out[:, Cs:].any()
        # unpad drops the padded channels whatever they hold
        padded = exp.clone()
        padded[:, Cs:] = 5.0
        dst = nans((P, Cs))
        A.check(A.lib().sgg_unpad_channels(K._p(padded.cuda()), K._p(dst), P, Cd, Cs, K.dt(dtype), K._s()), "unpad_channels")
        assert not torch.isnan(dst).any() and torch.equal(dst.cpu(), exp[:, :Cs].float()), f"unpad P={P}"
        if name == "f32":
            assert torch.equal(K.unpad_channels(out, Cs).cpu(), src), "round trip"


# ---------------------------------------------------------------------------- argmax-u8 labels
def argmax_case(P, Cr, Cp, seed):
    rng = np.random.default_rng([51, P, Cr, Cp, seed])
    k = rng.integers(0, 256, (P, Cp)).astype(np.float32) / np.float32(255)
    near = np.stack([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1))])            # exact k/255 and its neighbours
    pool = np.array([-1.0, -0.3, -0.004, 1.0, 1.0 + 1 / 255, 1.2, 1.5, 2.0, 0.0, -0.0], np.float32)   # negatives, wrap-around
    x = rng.uniform(0, 1, (P, Cp)).astype(np.float32)
    pick = rng.integers(0, 4, (P, Cp))
    x = np.where(pick == 1, np.take_along_axis(near, rng.integers(0, 3, (1, P, Cp)), 0)[0], x)
    x = np.where(pick == 2, pool[rng.integers(0, len(pool), (P, Cp))], x)
    rows = np.arange(P)
    c1, c2 = rng.integers(0, Cr, P), rng.integers(0, Cr, P)
    tie = rng.integers(0, 4, P) == 0
    x[rows[tie], c2[tie]] = x[rows[tie], c1[tie]]                                                     # constructed ties
    flat = rng.integers(0, 16, P) == 0
    x[flat] = x[flat, :1]                                                                             # all-equal pixels
    x[0] = x[0, 0]
    return x


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("Cr,Cp", [(3, 8), (34, 40)])
def test_argmax_u8_labels(K, A, name, Cr, Cp):
    for P in (1, 257, 70000):
        tx = dev(argmax_case(P, Cr, Cp, 0), DT[name])
        xq = tx.float().cpu().numpy()
        labels = torch.full((P,), -1, dtype=torch.int32, device="cuda")
        A.check(A.lib().sgg_argmax_u8_labels(K._p(tx), K._p(labels), P, Cr, Cp, K.dt(tx), K._s()), "argmax_u8_labels")
        got, exp = labels.cpu().numpy(), S.argmax_u8(xq, Cr)
        assert (got >= 0).all(), "unwritten labels"
        assert np.array_equal(got, exp), (P, int((got != exp).sum()), np.argwhere(got != exp)[:3].tolist())
        assert len(np.unique(exp)) > 1 or P == 1


# ---------------------------------------------------------------------------- confusion histogram
@pytest.mark.parametrize("n_class", [8, 34])
def test_confusion_hist(K, A, n_class):
    rng = np.random.default_rng(61)

    def run(lt, lp, hist):
        tl, tp = (torch.as_tensor(v.astype(np.int32)).cuda() for v in (lt, lp))
        A.check(A.lib().sgg_confusion_hist(K._p(tl), K._p(tp), len(lt), n_class, K._p(hist), K._s()), "confusion_hist")

    for n in (1, 1000, 1024 * 256 + 77):                                       # the last: the grid-stride loop
        lt, lp = rng.integers(-1, n_class + 1, n), rng.integers(-1, n_class + 1, n)
        if n == 1:
            lt[:], lp[:] = 2, 7
        hist = torch.zeros(n_class * n_class, dtype=torch.int64, device="cuda")
        run(lt, lp, hist)
        exp = S.confusion_hist(lt, lp, n_class)
        assert np.array_equal(hist.cpu().numpy(), exp), n
        run(lt, lp, hist)                                                      # adds to what is there
        assert np.array_equal(hist.cpu().numpy(), 2 * exp), n
    n = 1024 * 256 + 77                                                        # every pixel into one cell: exact under contention
    hist = torch.zeros(n_class * n_class, dtype=torch.int64, device="cuda")
    run(np.full(n, 3), np.full(n, 5), hist)
    exp = np.zeros(n_class * n_class, np.int64); exp[3 * n_class + 5] = n
    assert np.array_equal(hist.cpu().numpy(), exp)


# ---------------------------------------------------------------------------- segmentation-edge indicator
def seg_edge_abi(K, A, seg, out, N, H, W, Cr=3):
    return A.lib().sgg_seg_edge_weight(K._p(seg), K._p(out), N, H, W, Cr, seg.shape[-1], K.dt(seg), K._s())


@pytest.mark.parametrize("name", NAMES)
def test_seg_edge_weight(K, A, name):
    dtype = DT[name]
    rng = np.random.default_rng(71)
    for H, W in ((2, 2), (2, 9), (9, 2), (17, 31)):
        seg = S.eighths(rng, (2, H, W, 8))                                     # padded channels vary everywhere: not looked at
        blocks = S.eighths(rng, (2, -(-H // 3), -(-W // 4), 3))
        seg[..., :3] = np.repeat(np.repeat(blocks, 3, 1), 4, 2)[:, :H, :W]     # two different blocky images
        ts = dev(seg, dtype)
        out = nans((2, H, W))
        A.check(seg_edge_abi(K, A, ts, out, 2, H, W), "seg_edge_weight")
        exp = S.seg_edge(seg, 3)
        same(out, exp, f"edge {H}x{W}")
        assert torch.equal(K.seg_edge_weight(ts, 3), out)
        assert H * W <= 4 or (exp.any() and not exp.all())
    # one pixel differs from a constant map in the SECOND image only: REFLECT decides which neighbours light up
    for h, w in ((0, 0), (4, 5), (0, 3), (2, 0), (2, 3), (1, 1)):
        seg = np.full((2, 5, 6, 8), 0.5)
        seg[1, h, w, 1] = 0.25
        out = nans((2, 5, 6))
        A.check(seg_edge_abi(K, A, dev(seg, dtype), out, 2, 5, 6), "seg_edge_weight")
        exp = S.seg_edge(seg, 3)
        same(out, exp, f"single pixel {(h, w)}")
        assert not exp[0].any() and exp[1].any()
    # a map with one row or one column has no REFLECT neighbour: rejected before the launch
    out = nans((2, 5, 6))
    ts = dev(np.zeros((2, 5, 6, 8)), dtype)
    assert seg_edge_abi(K, A, ts, out, 60, 1, 1) == A.EINVAL and seg_edge_abi(K, A, ts, out, 2, 1, 30) == A.EINVAL
    assert seg_edge_abi(K, A, ts, out, 2, 30, 1) == A.EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("grad_scale", [0.5, 0.125])
@pytest.mark.parametrize("n", [1, 10007, 2048 * 256 + 257])
def test_adam_grad_scale(K, grad_scale, n):
    """Three steps with grad_scale != 1 (the data-parallel 1/world); n past the 2048-block cap takes the grid-stride loop.
    theta: three f32 roundings of |theta| < 8 (2.4e-7 each) + the update's own error -- the 2e-6 of test_adam_tf_form; m and v
    at 1e-4 of their scale."""
    rng = np.random.default_rng(81)
    f = lambda a: a.astype(np.float32).astype(np.float64)
    th, m, v = f(rng.standard_normal(n)), np.zeros(n), np.zeros(n)
    tth, tm, tv = dev(th), dev(m), dev(v)
    for t in (1, 2, 3):
        g = f(rng.standard_normal(n) * 0.4)
        th, m, v = S.adam(th, g, m, v, t, 1e-3, 0.5, 0.999, 1e-7, grad_scale)
        K.adam(tth, dev(g), tm, tv, t, 1e-3, 0.5, 0.999, 1e-7, grad_scale)
    err = np.abs(host(tth) - th).max()
    print(f"adam n={n} gs={grad_scale}: theta max abs err {err:.3e}")
    assert err < 2e-6
    close(tm, m, torch.float32, "m"); close(tv, v, torch.float32, "v")
