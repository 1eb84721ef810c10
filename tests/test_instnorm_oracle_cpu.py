"""tests/instnorm_oracle.py without a GPU.

1. The float64 statement is pinned to two independent references -- oracle/sggan_oracle.py (instance_norm + relu / lrelu on a
   Tape) and torch CPU float64 autograd (torch.nn.functional.instance_norm) -- on several shapes, the three activations, the
   plain / residual / skip forms and the two-network form.
2. For EVERY case of tests/test_gpu_instnorm.py: the exact family's premise holds, the random family's pre-activations keep
   their margin from the kink, and a NumPy emulation of the arithmetic the header promises (float32 elementwise; float64
   sums rounded to float32 once per chunk on the f32 path, float32 sums on the bf16 path; one storage rounding) stays inside
   the derived bounds -- equals the oracle bit for bit on the exact family.  The reference alone meets every bound before a
   kernel is asked to.
3. partial_rows with one chunk and with many chunks finalises to the same statistics."""
import numpy as np
import pytest
import torch

from oracle import sggan_oracle as O
from tests import instnorm_oracle as I

F32, F64 = np.float32, np.float64
TOL = 1e-11
ACTS = [(I.NONE, 0.0), (I.RELU, 0.0), (I.LRELU, 0.3), (I.LRELU, 0.2)]
SPECS = I.all_specs()


def V(a):
    return O.Var(np.asarray(a, F64))


def _inputs(shape, seed):
    rng = np.random.default_rng(seed)
    C = shape[-1]
    x = rng.standard_normal(shape) * 1.5 + 0.3
    return (x, 1 + 0.2 * rng.standard_normal(C), 0.2 * rng.standard_normal(C), rng.standard_normal(shape), rng.standard_normal(shape),
            -1.5 + 0.2 * rng.standard_normal(C), 0.7 + 0.2 * rng.standard_normal(C))


# ---------------------------------------------------------------------------- 1. pinned to two references
@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (2, 3, 5, 8), (3, 8, 8, 16), (2, 19, 27, 8)])
@pytest.mark.parametrize("act,leak", ACTS)
@pytest.mark.parametrize("form", ["plain", "residual", "skip"])
def test_matches_sggan_oracle(shape, act, leak, form):
    x, gamma, beta, extra, dy, _, _ = _inputs(shape, [1, *shape, act])
    eps = 1e-3
    t = O.Tape()
    vx, vg, vb, ve = V(x), V(gamma), V(beta), V(extra)
    h = O.instance_norm(t, vx, vg, vb, I.f32(eps))
    if form == "skip":
        h = O.add(t, h, ve)
    if act == I.RELU:
        h = O.relu(t, h)
    elif act == I.LRELU:
        h = O.lrelu(t, h, I.f32(leak))
    if form == "residual":
        h = O.add(t, h, ve)
    t.backward([(h, dy)])
    kw = {"residual": extra} if form == "residual" else {"skip": extra} if form == "skip" else {}
    y, mean, rstd, _ = I.forward(x, gamma, beta, eps, act, leak, **kw)
    b = I.backward(dy, x, gamma, beta, mean, rstd, act, leak, skip=kw.get("skip"))
    assert np.abs(y - h.v).max() <= TOL
    assert np.abs(b["dx"] - vx.g).max() <= TOL and np.abs(b["dgamma"] - vg.g).max() <= TOL and np.abs(b["dbeta"] - vb.g).max() <= TOL
    if form == "skip":
        assert np.abs(b["dskip"] - ve.g).max() <= TOL


def _torch_in(x, gamma, beta, eps, act, leak, skip=None, residual=None):
    h = torch.nn.functional.instance_norm(x.permute(0, 3, 1, 2), weight=gamma, bias=beta, use_input_stats=True, eps=I.f32(eps)).permute(0, 2, 3, 1)
    if skip is not None:
        h = h + skip
    if act == I.RELU:
        h = torch.relu(h)
    elif act == I.LRELU:
        h = torch.nn.functional.leaky_relu(h, I.f32(leak))
    return h if residual is None else h + residual


@pytest.mark.parametrize("shape,nsplit", [((2, 3, 5, 8), None), ((3, 8, 8, 16), None), ((2, 4, 4, 8), 1), ((3, 8, 8, 8), 1), ((3, 8, 8, 8), 2)])
@pytest.mark.parametrize("act,leak", ACTS)
@pytest.mark.parametrize("form", ["plain", "residual", "skip"])
def test_matches_torch_float64_autograd(shape, nsplit, act, leak, form):
    """torch's instance_norm is biased and takes the same eps; the two-network form is one call per parameter set on the whole batch, each keeping its own images."""
    x, gamma, beta, extra, dy, gamma2, beta2 = _inputs(shape, [2, *shape, act])
    eps = 1e-3
    T = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    tx, tg, tb, te, tg2, tb2 = T(x), T(gamma), T(beta), T(extra), T(gamma2), T(beta2)
    kt = {"residual": te} if form == "residual" else {"skip": te} if form == "skip" else {}
    if nsplit is None:
        h = _torch_in(tx, tg, tb, eps, act, leak, **kt)
    else:
        # both parameter sets on the whole batch, then the images of each network picked out
        h = torch.cat([_torch_in(tx, tg, tb, eps, act, leak, **kt)[:nsplit], _torch_in(tx, tg2, tb2, eps, act, leak, **kt)[nsplit:]])
    h.backward(torch.tensor(dy))
    pair = None if nsplit is None else (gamma2, beta2, nsplit)
    kw = {"residual": extra} if form == "residual" else {"skip": extra} if form == "skip" else {}
    y, mean, rstd, _ = I.forward(x, gamma, beta, eps, act, leak, pair=pair, **kw)
    b = I.backward(dy, x, gamma, beta, mean, rstd, act, leak, skip=kw.get("skip"), pair=pair)
    n = lambda t_: t_.detach().numpy()
    assert np.abs(y - n(h)).max() <= TOL and np.abs(b["dx"] - n(tx.grad)).max() <= TOL
    assert np.abs(b["dgamma"] - n(tg.grad)).max() <= TOL and np.abs(b["dbeta"] - n(tb.grad)).max() <= TOL
    if nsplit is not None:
        assert np.abs(b["dgamma2"] - n(tg2.grad)).max() <= TOL and np.abs(b["dbeta2"] - n(tb2.grad)).max() <= TOL
    if form == "skip":
        assert np.abs(b["dskip"] - n(te.grad)).max() <= TOL
    # the statistics against the plain definition
    assert np.abs(mean - x.mean((1, 2))).max() <= TOL and np.abs(rstd - 1 / np.sqrt(x.var((1, 2)) + I.f32(eps))).max() <= TOL


def test_kink_convention():
    """Slope at a pre-activation of exactly 0: 0 for RELU, leak for LRELU."""
    z = np.array([-1.0, 0.0, 1.0])
    assert np.array_equal(I.slope(z, I.RELU, 0.0), [0, 0, 1]) and np.array_equal(I.slope(z, I.LRELU, 0.25), [0.25, 0.25, 1])
    assert np.array_equal(I.slope(z, I.NONE, 0.0), [1, 1, 1])


def test_storage_rounding_matches_torch():
    a = np.random.default_rng(3).standard_normal(4096) * np.exp(np.random.default_rng(4).uniform(-20, 20, 4096))
    exp = torch.tensor(a.astype(F32)).to(torch.bfloat16).float().numpy().astype(F64)
    assert np.array_equal(I.to_storage(a, "bf16"), exp) and np.array_equal(I.to_storage(a, "f32"), a.astype(F32).astype(F64))


def test_chunk_geometry_reaches_the_edges_it_claims():
    """The reasons quoted next to I.SHAPES."""
    assert [I.rows_per_chunk(h) for h in (512, 513, 1320, 8192, 8193, 133225, 524288, 524289)] == [64, 64, 64, 64, 128, 1088, 4096, 4096]
    assert [I.chunks(h) for h in (513, 1320, 8193, 133225, 524288, 524289)] == [9, 21, 65, 123, 128, 129]
    assert 513 % 64 == 1 and 1320 % 64 == 40 and 8193 % 128 == 1
    assert I.rows_per_block(1, 133225) == 65 and 133225 % 65 == 40 and -(-133225 // 65) == 2050
    assert I.rows_per_block(1, 524289) == 256 and -(-524289 // 256) == 2049
    assert I.rows_per_block(2, 1320) == 64 and I.rows_per_block(1, 131072) == 64 and I.rows_per_block(1, 133120) == 65
    assert 1032 // 4 == 258 and 2056 // 8 == 257
    assert max(np.prod(s[0]) * max(s[1].values()) * 4 for s in I.SHAPES) <= 17 << 20 and np.prod(I.BIG) * 4 <= 17 << 20


# ---------------------------------------------------------------------------- 2. emulation of the promised arithmetic
def emu_stats(x, eps, name, rpc):
    """(mean, rstd) float32 (N, C): per-chunk sums (f32 path: float64, rounded once; bf16 path: float32), float64 combination."""
    N, H, W, C = x.shape
    xs = x.reshape(N, H * W, C).astype(F32)
    s = np.zeros((2, N, C), F64)
    for p0 in range(0, H * W, rpc):
        blk = xs[:, p0:p0 + rpc]
        if name == "f32":
            b64 = blk.astype(F64)
            s[0] += b64.sum(1).astype(F32); s[1] += (b64 * b64).sum(1).astype(F32)
        else:
            s[0] += blk.sum(1, dtype=F32); s[1] += (blk * blk).sum(1, dtype=F32)
    mean = s[0] / (H * W)
    var = np.maximum(s[1] / (H * W) - mean * mean, 0.0)
    return mean.astype(F32), (1.0 / np.sqrt(var + F64(F32(eps)))).astype(F32)


def _par(case, N):
    p = case["pair"]
    g = I.per_image(case["gamma"], N, *(p[2], p[0]) if p else ()).astype(F32)
    b = I.per_image(case["beta"], N, *(p[2], p[1]) if p else ()).astype(F32)
    return g, b


def emu_forward(case, mean32, rstd32, name, residual=None, skip=None):
    x = case["x"].astype(F32)
    gm, bt = _par(case, x.shape[0])
    mu, rs = mean32[:, None, None, :], rstd32[:, None, None, :]
    A = gm * rs
    B = bt - mu * A
    z = x * A + B
    if skip is not None:
        z = z + skip.astype(F32)
    leak = F32(case["leak"])
    y = z if case["act"] == I.NONE else np.where(z > 0, z, F32(0) if case["act"] == I.RELU else leak * z)
    if residual is not None:
        y = y + residual.astype(F32)
    assert y.dtype == F32
    return I.to_storage(y, name)


def emu_backward(case, dy, mean32, rstd32, name, rpc, acc, y_skip=None):
    """acc: 'f32' (float64 sums, one rounding per chunk) or 'bf16' (float32 sums).  y_skip: the skip form's stored output --
    g is then dy * act'(y), stored to the tensor's type, and the sums run over the stored values."""
    x, dy = case["x"].astype(F32), dy.astype(F32)
    N, H, W, C = x.shape
    HW = H * W
    gm, bt = _par(case, N)
    mu, rs = mean32[:, None, None, :], rstd32[:, None, None, :]
    xh = (x - mu) * rs
    leak = F32(case["leak"])
    sl = lambda z: np.ones_like(z) if case["act"] == I.NONE else np.where(z > 0, F32(1), F32(0) if case["act"] == I.RELU else leak)
    if y_skip is None:
        g = dy * sl(gm * xh + bt)
        act_pre = gm * xh + bt
    else:
        g = I.to_storage(dy * sl(y_skip.astype(F32)), name).astype(F32)
        act_pre = None
    assert g.dtype == F32 and xh.dtype == F32
    gs, xs = g.reshape(N, HW, C), xh.reshape(N, HW, C)
    s = np.zeros((2, N, C), F64)
    for p0 in range(0, HW, rpc):
        a, b = gs[:, p0:p0 + rpc], xs[:, p0:p0 + rpc]
        if acc == "f32":
            s[0] += a.astype(F64).sum(1).astype(F32); s[1] += (a.astype(F64) * b.astype(F64)).sum(1).astype(F32)
        else:
            s[0] += a.sum(1, dtype=F32); s[1] += (a * b).sum(1, dtype=F32)
    m1, m2 = (s[0] / HW).astype(F32)[:, None, None, :], (s[1] / HW).astype(F32)[:, None, None, :]
    tot = s.astype(F32).astype(F64)
    A = gm * rs
    dx = A * ((g - m1) - xh * m2)
    assert dx.dtype == F32
    n1 = case["pair"][2] if case["pair"] else N
    out = {"dx": I.to_storage(dx, name), "dskip": g.astype(F64), "pre": act_pre,
           "dbeta": tot[0, :n1].sum(0).astype(F32).astype(F64), "dgamma": tot[1, :n1].sum(0).astype(F32).astype(F64)}
    if case["pair"]:
        out["dbeta2"], out["dgamma2"] = tot[0, n1:].sum(0).astype(F32).astype(F64), tot[1, n1:].sum(0).astype(F32).astype(F64)
    return out


def _inside(got, exp, bound, what):
    err = np.abs(np.asarray(got, F64) - exp)
    assert np.isfinite(err).all(), what
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} outside the bound, worst ratio {np.nanmax(err / np.maximum(bound, 1e-300)):.3g}"


def _same(got, exp, what):
    got, exp = np.asarray(got, F64), np.asarray(exp, F64)
    bad = got != exp
    assert not bad.any(), f"{what}: {int(bad.sum())} differ, first {got[bad][0]!r} vs {exp[bad][0]!r}"


@pytest.mark.parametrize("spec", SPECS, ids=[s["id"] for s in SPECS])
def test_every_gpu_case_premise_margin_and_reference_emulation(spec):
    case = I.build(spec)
    name, act, leak, eps, pair = spec["name"], case["act"], case["leak"], case["eps"], case["pair"]
    x = case["x"]
    N, H, W, C = x.shape
    HW = H * W
    exact = spec["family"] == "exact"
    assert np.array_equal(I.to_storage(x, name), x)
    mean, rstd = I.stats(x, eps)
    st32 = (mean.astype(F32), rstd.astype(F32))
    o_plain, o_skip = (I.exact_premise(case) if exact else
                       (I.backward(case["dy"], x, case["gamma"], case["beta"], mean, rstd, act, leak, None, pair),
                        I.backward(case["dy_skip"], x, case["gamma"], case["beta"], mean, rstd, act, leak, case["skip"], pair)))
    layouts = [(True, I.chain_pixels(HW, True))] + ([(False, I.chain_pixels(HW, False))] if HW <= I.FUSED_MAXHW and HW > 64 else [])
    for one_launch, rpc in layouts:
        rel = I.sum_rel(name, rpc)
        em, er = emu_stats(x, eps, name, rpc)
        if exact:
            _same(em, mean, "mean"); _same(er, rstd, "rstd")
        else:
            bm, br = I.stats_bounds(x, eps, rel)
            _inside(em, mean, bm, "mean"); _inside(er, rstd, br, "rstd")
        for form, kw in (("plain", {}), ("residual", {"residual": case["residual"]}), ("skip", {"skip": case["skip"]})):
            y = I.forward(x, case["gamma"], case["beta"], eps, act, leak, pair=pair, **kw)[0]
            ey = emu_forward(case, em, er, name, **kw)
            if exact:
                _same(ey, I.to_storage(y, name), f"y {form}")
            else:
                by, bpre = I.forward_bounds(x, case["gamma"], case["beta"], eps, act, leak, name, rel, pair=pair, **kw)
                _inside(ey, y, by, f"y {form}")
                if act != I.NONE and form != "residual":
                    pre = I.forward(x, case["gamma"], case["beta"], eps, act, leak, pair=pair, **kw)[3]
                    assert (np.abs(pre) >= I.MARGIN * bpre).all(), f"{form}: a pre-activation is within {I.MARGIN} forward bounds of the kink"
        # backward, handed the oracle's statistics rounded to float32
        runs = [("plain", case["dy"], name, None, o_plain)]
        if name == "bf16":                                          # f32 gradient of a bf16 tensor: float32 sums, bf16 store
            runs.append(("mixed", case.get("dy32", case["dy"]), "bf16", None, None))
        y_skip = I.to_storage(I.forward(x, case["gamma"], case["beta"], eps, act, leak, skip=case["skip"], pair=pair)[0], name)
        runs.append(("skip", case["dy_skip"], name, y_skip, o_skip))
        for form, dy, acc, ys, o in runs:
            skip = case["skip"] if form == "skip" else None
            if o is None:
                o = I.backward(dy, x, case["gamma"], case["beta"], mean, rstd, act, leak, None, pair)
            e = emu_backward(case, dy, *st32, name, rpc, acc, ys)
            keys = [k for k in ("dx", "dgamma", "dbeta", "dgamma2", "dbeta2") if k in o] + (["dskip"] if form == "skip" else [])
            if exact:
                for k in keys:
                    _same(e[k], I.to_storage(o[k], name) if k in ("dx", "dskip") else o[k], f"{form} {k}")
            else:
                b = I.backward_bounds(dy, x, case["gamma"], case["beta"], mean, rstd, act, leak, name, rel, skip=skip, pair=pair,
                                      store_g=form == "skip")
                for k in keys:
                    _inside(e[k], o[k], b[k], f"{form} {k}")
                if e["pre"] is not None and act != I.NONE:
                    assert ((e["pre"] > 0) == (o["pre"] > 0)).all(), "the float32 pre-activation changes side"
                    _inside(e["pre"], o["pre"], b["bpre"], f"{form} pre-activation")


@pytest.mark.parametrize("spec", I.specs_of("degenerate"), ids=[s["id"] for s in I.specs_of("degenerate")])
def test_degenerate_channels_are_what_they_claim(spec):
    case = I.build(spec)
    x = case["x"]
    mean, rstd = I.stats(x, case["eps"])
    assert (x[..., 0].var((1, 2)) == 0).all() and (x[..., 1].var((1, 2)) == 0).all()
    assert np.allclose(rstd[:, :2], 1 / np.sqrt(I.f32(case["eps"])), rtol=1e-12)
    if spec["name"] == "f32":                                       # 1000.1 is no short float32: 40 of them do not sum exactly
        v = F32(x[0, 0, 0, 1])
        assert F64(F32(F64(v) * 40)) != F64(v) * 40
    assert np.abs(mean[:, 2] - 50).max() < 0.5 and np.abs(x[..., 2].std((1, 2)) - 0.5).max() < 0.2
    # the bound of the large-mean channel is wider than its neighbours' -- and finite
    bm, br = I.stats_bounds(x, case["eps"], I.sum_rel(spec["name"], 64))
    assert np.isfinite(br).all() and (br[:, 2] / rstd[:, 2] > 10 * br[:, 3] / rstd[:, 3]).all()


# ---------------------------------------------------------------------------- 3. statistics rows
@pytest.mark.parametrize("nchunks", (1,) + I.CHUNK_COUNTS[1:])
def test_partial_rows_finalise_to_the_same_statistics(nchunks):
    for spec in I.specs_of("chunks"):
        case = I.build(spec)
        x, eps = case["x"], case["eps"]
        HW = x.shape[1] * x.shape[2]
        mean, rstd = I.stats(x, eps)
        rows1, rows = I.partial_rows(x, 1), I.partial_rows(x, nchunks)
        assert rows.shape == (x.shape[0], nchunks, x.shape[3], 2) and rows.dtype == F32
        m1, r1 = I.finalize(rows1, HW, eps)
        m, r = I.finalize(rows, HW, eps)
        if spec["family"] == "exact":
            for a in (m1, m):
                _same(a, mean, "mean")
            for a in (r1, r):
                _same(a, rstd, "rstd")
        else:
            bm, br = I.stats_bounds(x, eps, I.U32, k=1.0)
            for a, b_ in ((m1, r1), (m, r)):
                _inside(a, mean, bm, "mean"); _inside(b_, rstd, br, "rstd")
        # the backward rows sum to the oracle's totals
        o = I.backward(case["dy"], x, case["gamma"], case["beta"], mean, rstd, case["act"], case["leak"])
        brow = I.bwd_partial_rows(case["dy"], x, case["gamma"], case["beta"], mean, rstd, case["act"], case["leak"], nchunks)
        assert np.abs(brow.astype(F64).sum((0, 1))[:, 0] - o["dbeta"]).max() <= 1e-4 * max(1, np.abs(o["dbeta"]).max())
        assert np.abs(brow.astype(F64).sum((0, 1))[:, 1] - o["dgamma"]).max() <= 1e-4 * max(1, np.abs(o["dgamma"]).max())


@pytest.mark.parametrize("shape", [(1, 8, 8, 8), (1, 3, 2731, 8), (1, 365, 365, 8)])
def test_eighths_family_keeps_the_forward_sums_exact(shape):
    x = I.eighths_case(*shape)
    I.eighths_premise(x, I.rows_per_chunk(shape[1] * shape[2]))
    I.eighths_premise(x[:, :1, :4096 if shape[2] >= 4096 else shape[2]], 4096)
    rows = I.partial_rows(x, I.chunks(shape[1] * shape[2]))
    assert np.array_equal(rows.astype(F64).sum(1)[..., 0], x.sum((1, 2))) and np.array_equal(rows.astype(F64).sum(1)[..., 1], (x * x).sum((1, 2)))
