"""Float64 statement of ``metric.dense_crf`` (reference metric.py:49-69), written twice.

pydensecrf is not available to this build, so the semantics below follow its published behaviour; every such point is
tagged [3P-recall].  Deviation: the message passing is EXACT -- every pixel pair -- where pydensecrf filters
through a permutohedral lattice, so parity with pydensecrf's own numbers is unpinned.

  [3P-recall] unary_from_softmax: U = -log(clip(p, 1e-5, 1.0)) as float32, shape (C, N), N = H*W row major.
  [3P-recall] addPairwiseGaussian(sxy, compat): features (x, y) / sxy, weight compat.
  [3P-recall] addPairwiseBilateral(sxy, srgb, rgbim, compat): features (x/sxy, y/sxy, r/srgb, g/srgb, b/srgb), weight compat.
  [3P-recall] both kernels are k(i,j) = exp(-0.5 |f_i - f_j|^2) and the sum over j includes j = i.
  [3P-recall] a scalar compat is the Potts model: the message of a label raises that label's own score by compat * message.
  [3P-recall] NORMALIZE_SYMMETRIC (the default of both add* calls): n_i = 1/sqrt(sum_j k(i,j) + 1e-20), filtered = n * (K (n * Q)).
  [3P-recall] inference(n): Q_0 = softmax_c(-U);  Q_{t+1} = softmax_c(-U + w_g M_g(Q_t) + w_b M_b(Q_t)), n times.
  Constants (metric.py:11-16): MAX_ITER 10, POS_W 3, POS_XY_STD 1, Bi_W 4, Bi_XY_STD 67, Bi_RGB_STD 3.

``dense_crf_matrix`` forms the two N x N kernels; ``dense_crf_loop`` walks the pixels one at a time and never holds more than
one kernel row.  tests/test_crf_cpu.py pins them to each other at 1e-12.  ``dense_crf_matrix(dtype=np.float32)`` is the same
formula in NumPy float32: its distance from the float64 result is the formula's own f32 error (eps32) that the GPU bound is a
multiple of.  The module also builds the seeded inputs the CPU and GPU tests share, and caches every result.
"""
import functools
import json
import os

import numpy as np

MAX_ITER, POS_W, POS_XY_STD, Bi_W, Bi_XY_STD, Bi_RGB_STD = 10, 3, 1, 4, 67, 3
PARAMS = dict(max_iter=MAX_ITER, pos_w=POS_W, pos_xy_std=POS_XY_STD, bi_w=Bi_W, bi_xy_std=Bi_XY_STD, bi_rgb_std=Bi_RGB_STD)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crf_eps32.json")


def unary_from_softmax(probs):
    """(C, H, W) -> float32 (C, N)."""
    p = np.asarray(probs)
    return (-np.log(np.clip(p.astype(np.float64), 1e-5, 1.0))).astype(np.float32).reshape(p.shape[0], -1)


def _softmax0(x):
    e = np.exp(x - x.max(axis=0, keepdims=True))
    return e / e.sum(axis=0, keepdims=True)


def dense_crf_matrix(img, probs, unary=None, dtype=np.float64, max_iter=MAX_ITER, pos_w=POS_W, pos_xy_std=POS_XY_STD, bi_w=Bi_W,
                     bi_xy_std=Bi_XY_STD, bi_rgb_std=Bi_RGB_STD):
    """Dense statement: img (H, W, 3) uint8, probs (C, H, W) (or a ready unary (C, N)) -> Q (C, H, W) in ``dtype``."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    U = (unary_from_softmax(probs) if unary is None else np.asarray(unary, dtype=np.float32)).astype(dtype)
    C = U.shape[0]
    yy, xx = np.mgrid[0:H, 0:W]
    xy = np.stack([xx.ravel(), yy.ravel()], axis=1).astype(dtype)
    rgb = img.reshape(-1, 3).astype(dtype)
    feats = (xy / dtype(pos_xy_std), np.concatenate([xy / dtype(bi_xy_std), rgb / dtype(bi_rgb_std)], axis=1))
    Ks, ns = [], []
    for F in feats:
        d2 = np.zeros((H * W, H * W), dtype=dtype)
        for d in range(F.shape[1]):
            diff = F[:, None, d] - F[None, :, d]
            d2 += diff * diff
        K = np.exp(dtype(-0.5) * d2)
        Ks.append(K)
        ns.append(dtype(1) / np.sqrt(K.sum(axis=1) + dtype(1e-20)))
    Q = _softmax0(-U)
    for _ in range(max_iter):
        msg = [n[None, :] * ((Q * n[None, :]) @ K.T) for K, n in zip(Ks, ns)]
        Q = _softmax0(-U + dtype(pos_w) * msg[0] + dtype(bi_w) * msg[1])
    return Q.reshape(C, H, W)


def dense_crf_loop(img, probs, unary=None, max_iter=MAX_ITER, pos_w=POS_W, pos_xy_std=POS_XY_STD, bi_w=Bi_W, bi_xy_std=Bi_XY_STD,
                   bi_rgb_std=Bi_RGB_STD):
    """The same, one target pixel at a time (float64): no N x N array exists at any point."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    N = H * W
    U = (unary_from_softmax(probs) if unary is None else np.asarray(unary, dtype=np.float32)).astype(np.float64)
    C = U.shape[0]
    px = np.arange(N) % W
    py = np.arange(N) // W
    col = img.reshape(N, 3).astype(np.float64)

    def rows(i):
        dist = (px - px[i]) ** 2 + (py - py[i]) ** 2                      # integer, exact
        colour = ((col - col[i]) ** 2).sum(axis=1)
        kg = np.exp(-dist / (2.0 * pos_xy_std ** 2))
        kb = np.exp(-dist / (2.0 * bi_xy_std ** 2) - colour / (2.0 * bi_rgb_std ** 2))
        return kg, kb

    ng, nb = np.empty(N), np.empty(N)
    for i in range(N):
        kg, kb = rows(i)
        ng[i] = 1.0 / np.sqrt(kg.sum() + 1e-20)
        nb[i] = 1.0 / np.sqrt(kb.sum() + 1e-20)
    Q = np.empty((C, N))
    for i in range(N):
        e = np.exp(-U[:, i] - (-U[:, i]).max())
        Q[:, i] = e / e.sum()
    for _ in range(max_iter):
        Qg, Qb = Q * ng, Q * nb
        new = np.empty_like(Q)
        for i in range(N):
            kg, kb = rows(i)
            logit = -U[:, i] + pos_w * ng[i] * (Qg @ kg) + bi_w * nb[i] * (Qb @ kb)
            e = np.exp(logit - logit.max())
            new[:, i] = e / e.sum()
        Q = new
    return Q.reshape(C, H, W)


# ---- the shared test inputs ----------------------------------------------------------------------------------------------
# name -> (H, W, C, kind, seed).  Shapes: under one tile both ways; channel padding (34 -> 40); several target and source
# tiles with a ragged tail on both; exact tile multiples.  One smooth-probability input, where the CRF moves labels.
CASES = {
    "tiny3": (12, 20, 3, "onehot", 11),
    "tiny34": (12, 20, 34, "onehot", 12),
    "ragged34": (33, 47, 34, "onehot", 13),
    "mult5": (32, 64, 5, "onehot", 14),
    "smooth3": (12, 20, 3, "smooth", 15),
}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(img uint8 (H,W,3), probs float32 (C,H,W)): blocky label map (4 x 4 blocks), image = palette[label] + noise, so colour
    edges sit on label edges; probs one-hot, or a smooth field peaked at the label."""
    H, W, C, kind, seed = CASES[name]
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, C, ((H + 3) // 4, (W + 3) // 4))
    labels = np.repeat(np.repeat(blocks, 4, axis=0), 4, axis=1)[:H, :W]
    palette = rng.integers(0, 256, (C, 3))
    img = np.clip(np.rint(palette[labels] + rng.normal(0.0, 2.0, (H, W, 3))), 0, 255).astype(np.uint8)
    if kind == "onehot":
        probs = (np.arange(C)[:, None, None] == labels[None]).astype(np.float32)
    else:
        yy, xx = np.mgrid[0:H, 0:W]
        field = np.stack([np.sin(0.37 * (c + 1) * xx + c) + np.cos(0.23 * (c + 2) * yy - c) for c in range(C)])
        logits = field + 1.5 * (np.arange(C)[:, None, None] == labels[None]) + rng.normal(0.0, 0.5, (C, H, W))
        probs = _softmax0(logits).astype(np.float32)
    img.setflags(write=False)
    probs.setflags(write=False)
    return img, probs


@functools.lru_cache(maxsize=None)
def case_q64(name):
    q = dense_crf_matrix(*case_inputs(name))
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def case_q32(name):
    q = dense_crf_matrix(*case_inputs(name), dtype=np.float32)
    q.setflags(write=False)
    return q


def measured_eps32():
    """{case: max |Q_f32 - Q_f64|} of the matrix statement over the shared inputs."""
    return {n: float(np.abs(case_q32(n).astype(np.float64) - case_q64(n)).max()) for n in CASES}


def golden_eps32():
    """The committed eps32: the largest entry of measured_eps32() when the fixture was written."""
    with open(GOLDEN) as f:
        return float(json.load(f)["eps32"])


def top2_margin(q):
    """(H, W): best minus second-best class probability."""
    s = np.sort(np.asarray(q, dtype=np.float64), axis=0)
    return s[-1] - s[-2]


def scores_mask_sample_crf_numpy(seg_mask_64, rescaled_sample, crf):
    """metric.py:79-89 with ``crf(img, probs)`` in place of dense_crf.  The mask is transposed to (1, C, W, H) and the image is
    not; the image's buffer is read as (W, H, 3), which is what it is when H == W."""
    sample_uint = rescaled_sample.astype(np.uint8)
    mask_uint = seg_mask_64.astype(np.uint8).transpose(0, 3, 2, 1)
    crf_labels = np.argmax(mask_uint, axis=1)
    h, w = mask_uint.shape[2:]
    q = crf(np.ascontiguousarray(sample_uint[0]).reshape(h, w, 3), mask_uint[0])
    return crf_labels, np.expand_dims(np.argmax(q, axis=0), axis=0), q


def write_golden():
    eps = measured_eps32()
    with open(GOLDEN, "w") as f:
        json.dump({"eps32": max(eps.values()), "per_case": eps,
                   "what": "max |Q_float32 - Q_float64| of tests/crf_oracle.dense_crf_matrix over crf_oracle.CASES"}, f, indent=1)
        f.write("\n")
    return eps


if __name__ == "__main__":
    print(write_golden())
