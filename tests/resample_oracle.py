"""float64 oracle of the input pipeline's resample (test infrastructure; the package never imports it).

skimage.transform.resize (0.16.2, order=1, mode='reflect', anti_aliasing=True) restated with SciPy: per axis with scale
s = n_in / n_out >= 1, ``gaussian_filter1d(sigma=(s-1)/2, mode='mirror', truncate=4.0)`` then explicit linear interpolation at
x_src = (x_dst + 0.5) * s - 0.5.  ``load_train`` / ``load_test`` chain the calls as utils.py:167-233 / 116-122 do.
``dense_*`` is a second statement of the same thing: the 1-D operator applied to an identity gives each axis' dense matrix,
the chain is their product, and the image is transformed by two matrix products.
"""
import numpy as np
from scipy.ndimage import gaussian_filter1d


def resize_axis(x, n_out, axis):
    x = np.asarray(x, dtype=np.float64)
    n_in = x.shape[axis]
    s = n_in / n_out
    if s < 1:
        raise ValueError("upscaling is out of scope")
    sigma = (s - 1.0) / 2.0
    if sigma > 0:
        x = gaussian_filter1d(x, sigma, axis=axis, mode="mirror", truncate=4.0)
    pos = (np.arange(n_out) + 0.5) * s - 0.5
    assert pos.min() >= 0 and pos.max() <= n_in - 1          # the warp's own boundary rule is never exercised
    x0 = np.floor(pos).astype(np.int64)
    f = pos - x0
    x1 = np.minimum(x0 + 1, n_in - 1)
    shape = [1] * x.ndim
    shape[axis] = n_out
    f = f.reshape(shape)
    return np.take(x, x0, axis=axis) * (1.0 - f) + np.take(x, x1, axis=axis) * f


def resize(x, hw):
    return resize_axis(resize_axis(x, hw[0], 0), hw[1], 1)


def as_float(u8):
    assert u8.dtype == np.uint8
    return u8.astype(np.float64) / 255.0


def load_train(u8, H, W):
    """utils.py:172-173 + 195-196: resize(x, (H0, H0)) then resize(x, (H, W)), float64 in between."""
    H0 = u8.shape[0]
    return resize(resize(as_float(u8), (H0, H0)), (H, W))


def load_test(u8, H, W):
    return resize(as_float(u8), (H, W))


def dense_axis(sizes):
    M = np.eye(sizes[0])
    for a, b in zip(sizes[:-1], sizes[1:]):
        M = resize_axis(np.eye(a), b, 0) @ M
    return M


def dense_apply(u8, row_sizes, col_sizes):
    R, C = dense_axis(row_sizes), dense_axis(col_sizes)
    return np.einsum("ih,hwc,jw->ijc", R, as_float(u8), C, optimize=True)


def epoch_protocol(files, epochs, batch_size, train_size, rng):
    """Literal restatement of model.py:219-228 + utils.py:201 with glob replaced by the sorted list: per epoch a fresh list
    is shuffled, min(len, train_size) // batch_size batches are cut, one flip draw per sample in batch order."""
    out = []
    for epoch in range(epochs):
        dataA = list(files)
        rng.shuffle(dataA)
        batch_idxs = min(len(dataA), train_size) // batch_size
        ep = []
        for idx in range(0, batch_idxs):
            batch_files = list(zip(dataA[idx * batch_size:(idx + 1) * batch_size]))
            ep.append([(bf[0], rng.random_sample() > 0.5) for bf in batch_files])
        out.append(ep)
    return out
