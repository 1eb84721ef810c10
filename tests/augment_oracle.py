"""float64 oracle of the augmented training copy's warp (test infrastructure; the package never imports it).

The rule of sggan_amd/data.py (deviation D6) stated a second time, as SEQUENTIAL coordinate maps instead of composite
matrices: an output pixel centre is carried through the output -> input map of the last applied operation, then the one before
it, down to the first; the zero-fill decision is taken where the point leaves the affine operation; the squared image is then
sampled once, bilinearly, with edge clamp.
"""
import numpy as np

FLIP, CROP, AFFINE = 0, 1, 2


def one(params, i):
    """Sample i of a draw_augment_params dict as plain Python values."""
    return {"perm": [int(v) for v in params["perm"][i]], "flip": bool(params["flip"][i]), "crop": [float(v) for v in params["crop"][i]],
            "translate": [float(v) for v in params["translate"][i]], "angle": float(params["angle"][i])}


def source_points(p, S):
    """-> (x, y, inside): where every output pixel centre of an S x S image samples the squared image, and whether the affine
    operation found its own source point inside its input image."""
    y, x = np.meshgrid(np.arange(S) + 0.5, np.arange(S) + 0.5, indexing="ij")
    inside = np.ones((S, S), dtype=bool)
    for op in reversed(p["perm"]):                      # the operation applied to the image last maps the output first
        if op == FLIP:
            if p["flip"]:
                x = S - x
        elif op == CROP:
            t, r, b, l = (float(np.rint(f * S)) for f in p["crop"])
            x = l + x * ((S - l - r) / S)
            y = t + y * ((S - t - b) / S)
        else:                                           # inverse of: rotate about the centre, then translate
            th = np.deg2rad(p["angle"])
            qx, qy = x - p["translate"][0] * S - S / 2.0, y - p["translate"][1] * S - S / 2.0
            x = np.cos(th) * qx + np.sin(th) * qy + S / 2.0
            y = -np.sin(th) * qx + np.cos(th) * qy + S / 2.0
            inside = (x >= 0) & (x <= S) & (y >= 0) & (y <= S)
    return x, y, inside


def bilinear(A, x, y):
    """A (S, S, C) sampled at continuous points (pixel centres at +0.5), neighbours clamped to the image."""
    S = A.shape[0]
    u, v = x - 0.5, y - 0.5
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fx, fy = (u - x0)[..., None], (v - y0)[..., None]
    c = lambda i: np.clip(i, 0, S - 1)
    top = A[c(y0), c(x0)] * (1 - fx) + A[c(y0), c(x0 + 1)] * fx
    bot = A[c(y0 + 1), c(x0)] * (1 - fx) + A[c(y0 + 1), c(x0 + 1)] * fx
    return top * (1 - fy) + bot * fy


def warp(A, p):
    """-> (warped (S, S, C) float64, inside (S, S) bool)."""
    A = np.asarray(A, dtype=np.float64)
    x, y, inside = source_points(p, A.shape[0])
    return np.where(inside[..., None], bilinear(A, x, y), 0.0), inside


def extremes():
    """Parameter sets at both ends of every range, for all six orders: (perm, flip, crop x 4, translate x 2, angle)."""
    import itertools
    sets = []
    for perm in itertools.permutations(range(3)):
        for hi in (False, True):
            sets.append({"perm": list(perm), "flip": hi, "crop": [0.4 if hi else 0.2] * 4,
                         "translate": [0.1 if hi else -0.1] * 2, "angle": 1.0 if hi else -1.0})
        # opposite ends mixed: wide crop with the largest shift one way and the other, rotation against the shift
        sets.append({"perm": list(perm), "flip": True, "crop": [0.2, 0.4, 0.4, 0.2], "translate": [0.1, -0.1], "angle": -1.0})
    return sets


def stack(sets):
    """A list of per-sample dicts -> the dict of arrays data.augment_matrices takes."""
    return {"perm": np.array([s["perm"] for s in sets], dtype=np.int64), "flip": np.array([s["flip"] for s in sets], dtype=bool),
            "crop": np.array([s["crop"] for s in sets], dtype=np.float64), "translate": np.array([s["translate"] for s in sets], dtype=np.float64),
            "angle": np.array([s["angle"] for s in sets], dtype=np.float64), "loader_flip": np.zeros(len(sets), dtype=bool)}
