"""The input-pipeline kernels -- sgg_resample_u8, sgg_resample_f32 (csrc/resample.hip), sgg_warp_affine_u8 (csrc/warp.hip) --
against tests/data_kernels_oracle.py at the sizes where their tiling changes path: ragged row blocks and column tiles, every
class of staged rows per chunk (rq) down to the refusal, every 16-byte alignment of a staged row including pieces that straddle
either end of the source buffer, degenerate bands, and for the warp ragged tiles, clamped windows, clamped origins and tiles
that lie wholly outside.

Every comparison is for EQUALITY: synthetic band tables in sixteenths, uint8 / k/256 sources and dyadic matrices make the
kernels' float32 arithmetic exact up to one correctly rounded division by 255 (tests/test_data_kernels_oracle_cpu.py proves
it for each case used here, and that each case selects the path it is named for).  Outputs are pre-filled with NaN and must be
written in full; padding channels must be exactly zero; a refused launch must leave its output untouched."""
import numpy as np
import pytest
import torch

from sggan_amd import _abi as A
from sggan_amd import data as D
from sggan_amd import kernels as K
from tests import data_kernels_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = (torch.float32, torch.bfloat16)


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def nans(shape, dtype=torch.float32):
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device=DEV)


def up(x, dtype=None):
    return torch.as_tensor(np.array(x, dtype=dtype, order="C")).to(DEV)            # a copy: the oracle's arrays are read-only


def same(got, exp, what=""):
    """Equality of values with no NaN on either side (+0 == -0); reports how many differ and where the first one is."""
    g, e = host(got) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64), np.asarray(exp, np.float64)
    assert g.shape == e.shape, (what, g.shape, e.shape)
    assert not np.isnan(g).any(), f"{what}: {int(np.isnan(g).sum())} unwritten (NaN) elements, first at {np.argwhere(np.isnan(g))[0].tolist()}"
    bad = g != e
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}: got {g[bad][0]!r}, expected {e[bad][0]!r}"


def device_tables(name):
    _, _, rows, cols = O.build(name)
    return D._device_tables((O.kernel_table(rows), O.kernel_table(cols)), DEV)


def device_source(name):
    """-> (source tensor, the flat buffer it is a view of or None).  With an offset the source is buf[off:off + n] of a buffer
    of 255s that ends where the source ends."""
    c, src, _, _ = O.build(name)
    if c["kind"] == "f32" or c["off"] is None:
        return up(src), None
    off = c["off"]
    buf = torch.full((off + src.size,), 255, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[off:] = up(src.reshape(-1))
    view = buf[off:off + src.size].view(*src.shape)
    assert view.data_ptr() == buf.data_ptr() + off and view.is_contiguous()
    return view, buf


def run(name, C, dtype, out=None):
    c = O.CASES[name]
    src, buf = device_source(name)
    rows, cols = device_tables(name)
    out = nans((len(c["index"]), c["H"], c["W"], 8), dtype) if out is None else out
    flip = up(c["flip"], np.int32)
    try:
        if c["kind"] == "u8":
            K.resample_u8(src, up(c["index"], np.int32), flip, rows, cols, out, C)
        else:
            K.resample_f32(src, flip, rows, cols, out, C)
    finally:
        torch.cuda.synchronize()
    if buf is not None:
        assert bool((buf[:c["off"]] == 255).all())
    return out


def check(name):
    c = O.CASES[name]
    for C in c["C"]:
        out32, out16 = run(name, C, torch.float32), run(name, C, torch.bfloat16)
        same(out32, O.resample_expect(name, C), f"{name} C={C} f32")
        same(out16, O.resample_expect(name, C, bf16=True), f"{name} C={C} bf16")
        assert torch.equal(out16, out32.to(torch.bfloat16))                   # bf16 = RNE of the f32 result, bit for bit
        assert torch.count_nonzero(out32[..., C:]) == 0 and torch.count_nonzero(out16[..., C:]) == 0


def check_refused(name):
    c = O.CASES[name]
    assert c["expect"] == "refused"
    for dtype in DTYPES:
        out = nans((len(c["index"]), c["H"], c["W"], 8), dtype)
        with pytest.raises(A.SggError):
            run(name, c["C"][0], dtype, out=out)
        assert bool(torch.isnan(out).all()), f"{name}: a refused launch wrote to its output"


# ---------------------------------------------------------------------------- sgg_resample_u8
@pytest.mark.parametrize("name", O.names("u8", "single-"))
def test_resample_u8_single_pixel(name):
    """H0 = W0 = H = W = 1: the source is 3 or 4 bytes, every staged piece takes the byte-guarded path."""
    check(name)


@pytest.mark.parametrize("name", O.names("u8", "tail-"))
def test_resample_u8_tile_tails(name):
    """H in {7, 8, 9, 17} x W in {1, 63, 64, 65, 255, 256, 257, 513}: ragged last row blocks and column tiles, all three weight
    tile widths, bands that are no multiple of rq and bands that overlap between row blocks."""
    check(name)


@pytest.mark.parametrize("name", [n for n in O.names("u8", "rq-") if O.CASES[n]["expect"] != "refused"])
def test_resample_u8_every_rq_class(name):
    check(name)


@pytest.mark.parametrize("name", [n for n in O.names("u8", "rq-") if O.CASES[n]["expect"] == "refused"])
def test_resample_u8_refuses_what_does_not_fit_and_writes_nothing(name):
    check_refused(name)


@pytest.mark.parametrize("name", O.names("u8", "align-"))
def test_resample_u8_every_alignment_and_both_buffer_ends(name):
    """The source is an offset view of a buffer of 255s: equality with the oracle shows that no byte outside the view reaches a
    result, whatever the alignment of a staged row."""
    check(name)


@pytest.mark.parametrize("name", O.names("u8", "degen-"))
def test_resample_u8_degenerate_bands(name):
    check(name)


@pytest.mark.parametrize("name", O.names("u8", "flip-"))
def test_resample_u8_flip_over_a_ragged_tile(name):
    c = O.CASES[name]
    assert (c["index"], c["flip"]) == ([1, 1, 0, 0], [0, 1, 1, 0])
    check(name)
    for dtype in DTYPES:
        out = run(name, c["C"][0], dtype)
        assert torch.equal(out[1], out[0].flip(1)) and torch.equal(out[2], out[3].flip(1))     # flipped = unflipped reversed along W


# ---------------------------------------------------------------------------- sgg_resample_f32
@pytest.mark.parametrize("name", O.names("f32", "tail-") + O.names("f32", "degen-"))
def test_resample_f32_tile_tails(name):
    check(name)


@pytest.mark.parametrize("name", [n for n in O.names("f32", "rq-") if O.CASES[n]["expect"] != "refused"])
def test_resample_f32_every_rq_class(name):
    check(name)


@pytest.mark.parametrize("name", [n for n in O.names("f32", "rq-") if O.CASES[n]["expect"] == "refused"])
def test_resample_f32_refuses_what_does_not_fit_and_writes_nothing(name):
    check_refused(name)


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_resample_f32_channel_counts(C):
    name = "flip-f32-W257"
    for dtype in DTYPES:
        out = run(name, C, dtype)
        same(out, O.resample_expect(name, C, bf16=dtype == torch.bfloat16), f"{name} C={C} {dtype}")
    assert O.resample_expect(name, 4)[..., 3].any()                          # C = 4 carries the fourth channel


@pytest.mark.parametrize("name", ["flip-f32-W257", "tail-f32-H17-W257-TR1-TC1-rs0-cs1-Cs4-M3"])
def test_resample_f32_strided_destinations(name):
    """out = buf[1::2] (the copies' rows of a doubled batch): the even samples stay bit for bit as they were; and a sample
    stride larger than H * W * 8 that is no multiple of it: the gap stays as it was."""
    c = O.CASES[name]
    N, H, W, C = len(c["flip"]), c["H"], c["W"], c["C"][0]
    assert N >= 2
    for dtype in DTYPES:
        want = O.resample_expect(name, C, bf16=dtype == torch.bfloat16)
        buf = torch.full((2 * N, H, W, 8), 7.0, dtype=dtype, device=DEV)
        buf[1::2] = float("nan")
        run(name, C, dtype, out=buf[1::2])
        same(buf[1::2], want, f"{name} buf[1::2] {dtype}")
        assert torch.equal(buf[0::2], torch.full_like(buf[0::2], 7.0))
        n = H * W * 8
        flat = torch.full((N, n + 16), 5.0, dtype=dtype, device=DEV)
        flat[:, :n] = float("nan")
        out = flat.as_strided((N, H, W, 8), (n + 16, W * 8, 8, 1))
        run(name, C, dtype, out=out)
        same(out, want, f"{name} stride H*W*8+16 {dtype}")
        assert torch.equal(flat[:, n:], torch.full_like(flat[:, n:], 5.0))


# ---------------------------------------------------------------------------- sgg_warp_affine_u8
def warp(src, index, mats, tab, window, out=None):
    N, S = len(mats), src.shape[1]
    cols, = D._device_tables((O.kernel_table(tab),), DEV)
    out = nans((N, S, S, 4)) if out is None else out
    try:
        K.warp_affine_u8(up(src), up(index, np.int32), up(mats), cols, window, out)
    finally:
        torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("which", O.WARP_TABLES)
@pytest.mark.parametrize("S", O.WARP_S)
def test_warp_against_the_oracle(S, which):
    """Identity, flips, half-pixel and whole-pixel shifts, integer translations, fill map != sample map (all outside; every
    neighbour clamped to the last / first row and column), scale 1/2 (crop-like), scale 2 (window columns clamped to S), axis
    swaps (tall window, rows clamped to S): several samples with different matrices per launch, window from data.warp_window."""
    for Cs in (3, 4):
        src, tab = O.warp_source(S, Cs, which)
        squared = [O.squared_f32(img, tab) for img in src]
        for group, maps in O.warp_groups(S).items():
            mats = np.stack([m for _, m in maps])
            index = [(k + 1) % 2 for k in range(len(maps))] + [1]            # alternating, then the last source once more
            mats = np.concatenate([mats, mats[:1]])
            out = warp(src, index, mats, tab, D.warp_window(mats))
            assert not torch.isnan(out).any() and torch.count_nonzero(out[..., 3]) == 0      # written in full, channel 3 zero
            for k, (i, m) in enumerate(zip(index, mats)):
                what = f"S={S} {which} Cs={Cs} {group}/{(maps + maps[:1])[k][0]} (sample {k}, source {i})"
                same(out[k], O.warp_expect(squared[i], m), what)
            if group == "unit":
                same(out[0, ..., :3], squared[index[0]], f"S={S} {which} Cs={Cs}: identity = the squared image")


def test_warp_lds_limit():
    """A 64 x 64 window is exactly 64 KB: accepted, and right for maps of every window class at once.  65 x 65 is refused and
    the output is left untouched."""
    g = O.warp_groups(64)
    mats = np.stack([m for k in ("double", "swap", "half") for _, m in g[k]] + [g["unit"][0][1]])
    for Cs in (3, 4):
        src, tab = O.warp_source(64, Cs, O.WARP_TABLES[2])
        squared = [O.squared_f32(img, tab) for img in src]
        index = [k % 2 for k in range(len(mats))]
        out = warp(src, index, mats, tab, (64, 64))
        for k, (i, m) in enumerate(zip(index, mats)):
            same(out[k], O.warp_expect(squared[i], m), f"S=64 window 64x64 Cs={Cs} sample {k}")
        src, tab = O.warp_source(65, Cs, O.WARP_TABLES[2])
        out = nans((1, 65, 65, 4))
        with pytest.raises(A.SggError):
            warp(src, [0], O.IDENT[None, None].repeat(2, axis=1), tab, (65, 65), out=out)
        assert bool(torch.isnan(out).all())
