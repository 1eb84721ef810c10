"""tests/small_kernels_oracle.py without a GPU: the float64 statements are pinned to oracle/sggan_oracle.py where that has the
same operation (1e-12), and every exact-by-construction input of tests/test_gpu_small_kernels.py is shown to be exact: a
float32 evaluation in the kernel's documented order (float32 within a chunk / a block, double across them) equals the
float64 one bit for bit, and no partial sum needs more than 24 bits of its granule.  A construction that fails here is
redesigned here; the GPU tests then compare for equality."""
import numpy as np
import pytest

from oracle import sggan_oracle as O
from tests import small_kernels_oracle as S

TOL = 1e-12


def V(a):
    return O.Var(np.asarray(a, np.float64))


# ---------------------------------------------------------------------------- pinned to oracle/sggan_oracle.py
@pytest.mark.parametrize("shape", [(1, 1, 1, 3), (2, 3, 5, 3), (1, 4, 7, 10)])
def test_l1_matches_sggan_oracle(shape):
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal(shape), rng.standard_normal(shape)
    b.flat[::5] = a.flat[::5]                                    # ties: gradient 0
    t = O.Tape(); vb = V(b); l = O.l1_mean(t, a, vb); t.backward([(l, 2.5)])
    loss, db = S.l1_loss(a, b, shape[-1], weight=2.5)
    assert abs(loss - 2.5 * l.v) <= TOL and np.abs(db - vb.g).max() <= TOL
    # channel padding: the padded channels change nothing and get no gradient
    ap, bp = S.pad_channels(a, 16) + 3.0, S.pad_channels(b, 16) - 1.0
    ap[..., :shape[-1]], bp[..., :shape[-1]] = a, b
    loss_p, db_p = S.l1_loss(ap, bp, shape[-1], weight=2.5)
    assert loss_p == loss and np.array_equal(db_p[..., :shape[-1]], db) and not db_p[..., shape[-1]:].any()
    # gscale scales the gradient only
    loss_g, db_g = S.l1_loss(a, b, shape[-1], weight=2.5, gscale=0.5)
    assert loss_g == loss and np.abs(db_g - 0.5 * db).max() <= TOL


@pytest.mark.parametrize("label", [0.0, 1.0, S.f32(0.9)])
def test_bce_and_mse_match_sggan_oracle(label):
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.standard_normal(37) * 3, [30.0, -30.0, 100.0, -100.0, 0.0]])
    t = O.Tape(); vx = V(x); l = O.bce_logits_mean(t, vx, label); t.backward([(l, 0.5)])
    loss, dx = S.bce_logits(x, label, weight=0.5)
    assert np.isfinite(loss) and abs(loss - 0.5 * l.v) <= TOL * max(1, abs(l.v)) and np.abs(dx - vx.g).max() <= TOL
    t = O.Tape(); vx = V(x); l = O.mse_const_mean(t, vx, label); t.backward([(l, 0.5)])
    loss, dx = S.mse_const(x, label, weight=0.5)
    assert abs(loss - 0.5 * l.v) <= TOL * max(1, abs(l.v)) and np.abs(dx - vx.g).max() <= TOL * max(1, np.abs(vx.g).max())
    _, dx_g = S.mse_const(x, label, weight=0.5, gscale=0.25)
    assert np.abs(dx_g - 0.25 * dx).max() <= TOL


@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 1, 7), (1, 7, 1), (3, 2, 5), (2, 6, 9)])
def test_gradloss_matches_sggan_oracle(dims):
    rng = np.random.default_rng(3)
    C = 3
    a, b = rng.standard_normal(dims + (C,)), rng.standard_normal(dims + (C,))
    w = S.half_weights(rng, dims)
    t = O.Tape(); va = V(a); l = O.gradloss(t, va, b, w[..., None]); t.backward([(l, 5.0)])
    loss, din = S.gradloss(a, b, w, C, lam=5.0)
    assert abs(loss - 5.0 * l.v) <= TOL * max(1, abs(l.v)) and np.abs(din - va.g).max() <= TOL
    # the exact inputs hit sign(0) = 0 often: the two statements must agree there too
    a8, b8, w8, lam, _ = S.gradloss_case(*dims, C, C)
    t = O.Tape(); va = V(a8); l = O.gradloss(t, va, b8, w8[..., None]); t.backward([(l, lam)])
    loss, din = S.gradloss(a8, b8, w8, C, lam=lam)
    assert abs(loss - lam * l.v) <= TOL and np.abs(din - va.g).max() <= TOL


def test_seg_edge_matches_sggan_oracle_and_known_answers():
    rng = np.random.default_rng(4)
    for H, W in ((2, 2), (2, 9), (9, 2), (17, 31)):
        seg = rng.integers(0, 3, (2, H, W, 3)).astype(np.float64) / 2
        seg = np.repeat(np.repeat(seg, 2, 1), 2, 2)[:, :H, :W]
        assert np.array_equal(S.seg_edge(seg, 3), O.seg_edge_weight(seg)[..., 0])
    # one differing pixel in a constant 5 x 6 map.  A pixel is lit when its two neighbours along an axis differ.  REFLECT: a
    # border pixel has its inner neighbour on both sides (difference 0 along that axis)
    def lit(h, w):
        seg = np.zeros((1, 5, 6, 3)); seg[0, h, w, 1] = 1.0
        return {(int(i), int(j)) for i, j in zip(*np.nonzero(S.seg_edge(seg, 3)[0]))}
    assert lit(2, 3) == {(1, 3), (3, 3), (2, 2), (2, 4)}                 # interior: the four neighbours, not the pixel itself
    assert lit(0, 0) == {(0, 1), (1, 0)}                                 # corner: its two neighbours
    assert lit(0, 3) == {(0, 2), (0, 4), (1, 3)}                         # top edge: three neighbours
    assert lit(1, 1) == {(2, 1), (1, 2)}                                 # next to the corner: (0,1) and (1,0) see it on BOTH sides
    seg = np.zeros((1, 4, 4, 8)); seg[0, 1, 1, 5] = 1.0                  # a padded channel is not looked at
    assert not S.seg_edge(seg, 3).any()


def test_hist_argmax_adam_match_sggan_oracle():
    rng = np.random.default_rng(5)
    for n_class in (8, 34):
        lt = rng.integers(-1, n_class + 1, 500)
        lp = rng.integers(0, n_class, 500)
        assert np.array_equal(S.confusion_hist(lt, lp, n_class).reshape(n_class, n_class), O.fast_hist(lt, lp, n_class))
        bad = rng.integers(-1, n_class + 1, 500)                        # predictions out of range are dropped as well
        ok = (bad >= 0) & (bad < n_class)
        assert np.array_equal(S.confusion_hist(lt, bad, n_class), S.confusion_hist(lt[ok], bad[ok], n_class))
    img = rng.uniform(0, 1, (2, 5, 7, 3)).astype(np.float32)            # in [0, 1): the numpy cast is defined
    img[0, 0, 0] = 0.5                                                   # all equal: label 0
    img[0, 0, 1] = (0.25, 0.75, 0.75)                                    # tie: first maximum
    gts, _ = O.scores_seg_fake(img, img)
    assert np.array_equal(S.argmax_u8(img.reshape(-1, 3), 3).reshape(2, 5, 7), gts.transpose(0, 2, 1))
    x = np.array([[-0.5, 0.25, 0.0], [1.5, 0.9, 0.0], [1.0 + 1 / 255, 1 / 255, 0.0]], np.float32)
    #  -127 & 255 = 129 wins; 382 & 255 = 126 < 229; 256 & 255 = 0 < 1
    assert S.argmax_u8(x, 3).tolist() == [0, 1, 1]
    th, m, v = rng.standard_normal(50), np.zeros(50), np.zeros(50)
    th2, m2, v2 = th.copy(), m.copy(), v.copy()
    for t in (1, 2, 3):
        g = rng.standard_normal(50)
        th, m, v = S.adam(th, g, m, v, t, 1e-3, 0.5, 0.999, 1e-7, grad_scale=0.125)
        th2, m2, v2 = O.adam_tf(th2, g * 0.125, m2, v2, t, S.f32(1e-3), 0.5, S.f32(0.999), S.f32(1e-7))
    assert max(np.abs(th - th2).max(), np.abs(m - m2).max(), np.abs(v - v2).max()) <= TOL


def test_pad_unpad_and_activations():
    x = np.arange(12.0).reshape(4, 3) - 5
    p = S.pad_channels(x, 8)
    assert p.shape == (4, 8) and np.array_equal(p[:, :3], x) and not p[:, 3:].any()
    assert np.array_equal(S.unpad_channels(p, 3), x)
    y = np.array([-2.0, -0.0, 0.0, 3.0])
    assert S.act_fwd(y, "relu").tolist() == [0, 0, 0, 3] and S.act_bwd(np.ones(4), y, "relu").tolist() == [0, 0, 0, 1]
    assert np.allclose(S.act_fwd(y, "lrelu", 0.2), [-0.4, 0, 0, 3], atol=1e-7)
    assert np.allclose(S.act_bwd(np.full(4, 2.0), y, "lrelu", 0.3), [0.6, 0.6, 0.6, 2], atol=1e-7)   # y = 0 takes the leak (TF)
    assert np.array_equal(S.act_bwd(np.ones(4), np.tanh(y), "tanh"), 1 - np.tanh(y) ** 2)


# ---------------------------------------------------------------------------- the exactness premise of the GPU cases
def test_values_are_exact_in_bfloat16():
    import torch
    vals = np.concatenate([np.arange(-8, 9) / 8.0, [0.0, 0.5, 1.0]])
    t = torch.tensor(vals, dtype=torch.float64)
    assert torch.equal(t.to(torch.bfloat16).to(torch.float64), t)
    # differences, Sobel derivatives (8 taps, |coefficient| <= 2) and weighted per-pixel sums stay on the 1/16 grid below 2^8
    assert 16 * (4 * 2 * 8 * 2) < 2 ** 24


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bias_grad_cases_are_exact(dtype):
    cases = [(C, P) for C in S.BIAS_C[dtype] for P in S.BIAS_P] + [(8, S.BIAS_P_BIG)]
    for C, P in cases:
        dy = S.bias_case(C, P)
        got = S.exact_sum_premise(dy, S.chunk_groups(P, S.BG_ROWS), 1 / 8)
        assert np.array_equal(np.atleast_1d(got), S.colsum(dy, C))
        assert np.array_equal(np.float32(got).astype(np.float64), np.atleast_1d(got))       # the f32 result is the sum itself
    assert -(-S.BIAS_P_BIG // S.BG_ROWS) > 256
    # accumulate: integer contents + the sum stay exact in float32
    assert np.abs(S.colsum(S.bias_case(8, S.BIAS_P_BIG), 8)).max() + 64 < 2 ** 21


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_l1_cases_are_exact(dtype):
    cases = [(S.l1_pixels(nv, Cp, dtype), Cr, Cp) for Cr, Cp in S.L1_SHAPES for nv in S.L1_NVEC]
    if dtype == "f32":
        cases.append((S.L1_P_BIG, 3, 8))
        assert S.L1_P_BIG * 8 // 4 > 256 * S.L1_ROWS and (S.L1_P_BIG * 8 // 4) % S.L1_ROWS
    else:
        assert {S.l1_pixels(nv, 8, dtype) for nv in S.L1_NVEC} == set(S.L1_NVEC)            # bf16, Cpad 8: one vector per pixel
    for P, Cr, Cp in cases:
        a, b, weight, factor = S.l1_case(P, Cr, Cp)
        terms = S.l1_terms(a, b, Cr)
        total = S.exact_sum_premise(terms, S.chunk_groups(terms.size, S.L1_ROWS * S.VEC[dtype]), 1 / 8)
        assert total == S.l1_sum(a, b, Cr)
        # scale = (double)weight / (P * Cr) and the gradient magnitude (float)(weight * gscale / (P * Cr)) are powers of two
        assert np.float64(np.float32(weight)) / (P * Cr) == factor and np.log2(factor) == round(np.log2(factor))
        loss, db = S.l1_loss(a, b, Cr, weight, gscale=0.5)
        assert loss == total * factor and np.float64(np.float32(loss)) == loss
        assert set(np.unique(db)) <= {-0.5 * factor, 0.0, 0.5 * factor} and not db[..., Cr:].any()
        assert (np.sign(a - b)[..., :Cr] == 0).any()                                        # ties are present
        # accumulate_grad onto contents j * factor, |j| <= 8: still a short multiple of factor / 2
        assert 2 * 8 + 1 < 2 ** 8


@pytest.mark.parametrize("Cr,Cp", S.GL_VEC_SHAPES + S.GL_SCALAR_SHAPES)
def test_gradloss_cases_are_exact(Cr, Cp):
    for dims in S.GL_DIMS + (S.GL_DIMS_BIG,):
        a, b, w, lam, factor = S.gradloss_case(*dims, Cr, Cp)
        n = int(np.prod(dims))
        terms = S.gradloss_terms(a, b, w, Cr).ravel()
        total = S.exact_sum_premise(terms, S.grid_stride_groups(n, S.BLOCK, S.GL_BLOCKS), 1 / 16)
        assert np.float64(np.float32(lam)) == lam and lam / (n * 2.0 * Cr) == factor
        for gscale in (1.0, 0.5):
            loss, din = S.gradloss(a, b, w, Cr, lam, gscale)
            assert loss == total * factor and np.float64(np.float32(loss)) == loss
            # din: at most 18 products coef * K with coef in {0, +-1/2, +-1} * factor * gscale, |K| <= 2, sum |K| = 16: an integer
            # number of half factors below 2^6 -- exact in bfloat16, in any order; + contents j * factor, |j| <= 8, below 2^7
            q = din / (factor * gscale / 2)
            assert np.array_equal(q, np.round(q)) and np.abs(q).max() <= 32 and not din[..., Cr:].any()
    assert int(np.prod(S.GL_DIMS_BIG)) > S.GL_BLOCKS * S.BLOCK
    if len(S.GL_DIMS) > 3:                                           # the three images of the N = 3 case differ
        a = S.gradloss_case(3, 2, 5, Cr, Cp)[0]
        assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2])
