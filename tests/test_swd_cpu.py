"""The sliced Wasserstein distance of the test pass (--swd) without a GPU: the NumPy oracle's two statements of
every stage pinned to each other, answers that follow from the definition, the patch positions, the C ABI of csrc/swd.hip
(declarations, bindings, every refusal -- on host memory that is never dereferenced), the workspace formulas, the register
budget, the flags, and eps64, the number the GPU tolerances are multiples of."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from sggan_amd import _abi as A
from tests import swd_oracle as O
from tests.diffaug_oracle import philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the oracle against itself
@pytest.mark.parametrize("H,W,levels", [(16, 16, 1), (32, 48, 2), (64, 96, 3), (112, 176, 5), (224, 352, 6)])
def test_pyramid_separable_equals_direct_sum_in_reversed_order(H, W, levels):
    """Integer inputs: every intermediate is an exact dyadic rational, so the two summation orders agree to the bit."""
    img = np.random.default_rng(H + levels).integers(0, 256, (2, H, W, 3)).astype(np.uint8)
    sep, direct = O.pyramid(img, levels), O.pyramid(img, levels, direct=True)
    assert [l.shape for l in sep] == [(2, 3, H >> k, W >> k) for k in range(levels)]
    for a, b in zip(sep, direct):
        assert a.dtype == np.float64 and np.array_equal(a, b)
    # the finest Laplacian level of a smooth image is small against the image, the coarsest is the blurred image itself
    assert abs(sep[-1].mean() - img.mean()) < 2.0
    if levels > 1:
        assert np.abs(sep[0]).mean() < img.mean()


def test_pyramid_border_and_known_answers():
    assert O.mirror(np.array([-2, -1, 0, 6, 7, 8]), 7).tolist() == [2, 1, 0, 6, 5, 4]
    const = np.full((1, 16, 32, 3), 93, np.uint8)
    lv = O.pyramid(const, 2)
    assert np.array_equal(lv[0], np.zeros((1, 3, 16, 32))) and np.array_equal(lv[1], np.full((1, 3, 8, 16), 93.0))
    # up() of a single coarse sample at the far corner: Z[2w] -> Z[2w-2] adds the outer tap to the centre one, Z[2w+1] -> Z[2w-3] = 0
    x = np.zeros((1, 1, 4, 4))
    x[..., 3, 3] = 64.0
    u = O.up(x)
    assert u.shape == (1, 1, 8, 8) and u[0, 0, 6, 6] == 64.0 * (6 + 1) ** 2 / 64 and u[0, 0, 7, 7] == 64.0 * (4 + 4) ** 2 / 64
    assert u[0, 0, 5, 5] == 64.0 * 4 * 4 / 64 and u[0, 0, 4, 4] == 64.0 / 64 and not u[0, 0, :4, :4].any()
    assert O.default_levels(256, 512) == 5 and O.default_levels(128, 128) == 4 and O.default_levels(15, 64) == 0 and O.default_levels(16, 24) == 1


def test_quantise_rule():
    x = np.array([-1.0, 1.0, -3.0, 7.0, np.nan, 0.0, 0.999], np.float32)
    assert O.quantise(x).tolist() == [0, 255, 0, 255, 0, 127, 254]
    u = np.arange(6, dtype=np.uint8)
    assert O.quantise(u) is u


@pytest.mark.parametrize("patches,offset", [(1, 0), (2, 5), (33, 0)])
def test_descriptor_gather_fancy_equals_loops(patches, offset):
    lv = O.pyramid(np.random.default_rng(3).integers(0, 256, (2, 28, 44, 3)).astype(np.uint8), 3)
    for level, planar in enumerate(lv):
        a, b = O.descriptors(planar, level, patches, 19, offset), O.descriptors_loops(planar, level, patches, 19, offset)
        assert a.shape == (2 * patches, 147) and np.array_equal(a, b)
    # keyed by the image index: image 1 of a call at offset 5 is image 0 of a call at offset 6
    assert np.array_equal(O.descriptors(lv[0], 0, patches, 19, 5)[patches:], O.descriptors(lv[0][1:], 0, patches, 19, 6))


def test_positions_lie_inside_the_level_and_follow_the_words():
    for h, w in ((7, 11), (7, 7), (14, 22), (112, 176)):
        for g in (0, 5, (1 << 32) + 5):
            pos = O.positions(19, g, 2, 33, h, w)
            assert np.all((pos[:, 0] >= 3) & (pos[:, 0] < h - 3)) and np.all((pos[:, 1] >= 3) & (pos[:, 1] < w - 3))
            if h == 7:
                assert np.all(pos[:, 0] == 3)                   # the only centre
    assert np.array_equal(O.positions(19, (1 << 32) + 5, 2, 33, 14, 22), O.positions(19, 5, 2, 33, 14, 22))   # g = uint32(offset + i)
    r = philox4x32_10((5, 2, 3, 0), (19, 1))
    pos = O.positions(19, 5, 2, 8, 112, 176)
    assert pos[6].tolist() == [3 + ((r[0] * 106) >> 32), 3 + ((r[1] * 170) >> 32)]
    assert pos[7].tolist() == [3 + ((r[2] * 106) >> 32), 3 + ((r[3] * 170) >> 32)]
    # an odd count leaves words 2, 3 of the last block unused: the first patches are those of any longer draw
    assert np.array_equal(O.positions(19, 5, 2, 7, 112, 176), pos[:7])
    big = O.positions(19, 0, 0, 512, 112, 176)
    assert big[:, 0].min() < 8 and big[:, 0].max() > 103 and big[:, 1].min() < 8 and big[:, 1].max() > 167         # the whole range is used
    assert O.mulhi32(0, 106) == 0 and O.mulhi32(0xFFFFFFFF, 106) == 105 and O.mulhi32(0xFFFFFFFF, 1) == 0        # centres 3 .. h - 4
    assert not np.array_equal(O.positions(19, 0, 0, 8, 112, 176), O.positions(19, 0, 1, 8, 112, 176))
    assert not np.array_equal(O.positions(19, 0, 0, 8, 112, 176), O.positions(20, 0, 0, 8, 112, 176))
    # the key's second word is 1: not the draws of the augmentation's key (seed, 0)
    assert philox4x32_10((0, 0, 0, 0), (19, 1)) != philox4x32_10((0, 0, 0, 0), (19, 0))
    assert O.positions(19, 0, 0, 4, 112, 176).tolist() == KNOWN_POSITIONS


KNOWN_POSITIONS = [[67, 77], [77, 57], [66, 14], [5, 161]]          # key (19, 1), counter (0, 0, 0..1, 0), level 112 x 176


@pytest.mark.parametrize("M,D", [(3, 1), (33, 128), (768, 16)])
def test_normalise_project_sort_distance_second_statement(M, D):
    """The rest of the chain stated again -- np.std, a matrix product, a loop over directions -- to 1e-12."""
    a, b = O.case_descriptors(M, D)
    dirs = O.directions(D)
    assert dirs.dtype == np.float32 and dirs.shape == (147, D)
    assert np.allclose(np.linalg.norm(dirs.astype(np.float64), axis=0), 1.0, atol=1e-6)
    m = O.moments(a)
    d3 = a.astype(np.float64).reshape(M, 3, 49)
    assert np.allclose(m[:, 0], d3.mean(axis=(0, 2)), rtol=1e-12) and np.allclose(m[:, 1], d3.transpose(1, 0, 2).reshape(3, -1).std(axis=1), rtol=1e-12)
    z = O.normalise(a)
    z2 = ((d3 - m[None, :, 0, None]) / m[None, :, 1, None]).reshape(M, 147)
    assert np.abs(z - z2).max() <= 1e-12
    assert np.abs(z.reshape(M, 3, 49).mean(axis=(0, 2))).max() < 1e-9 and np.allclose(z.reshape(M, 3, 49).std(axis=(0, 2)), 1.0, atol=1e-9)
    p, mag = O.project(z, dirs)
    assert p.shape == (D, M) and np.abs(p - (z @ dirs.astype(np.float64)).T).max() <= 1e-12 * mag.max()
    q, _ = O.project(O.normalise(b), dirs)
    want = 1e3 * np.mean([np.mean(np.abs(np.sort(p[d]) - np.sort(q[d]))) for d in range(D)])
    got = O.distance(p, q)
    assert got > 0 and abs(got - want) <= 1e-12 * want
    assert abs(O.score(a, b, dirs) - got) == 0.0


def test_identical_sets_give_zero_and_a_constant_set_no_nan():
    c = O.image_case()
    dirs = O.directions(128)
    vals, mean = O.swd(c["fakes"], c["fakes"].copy(), 2, 11, dirs)
    assert vals == [0.0, 0.0] and mean == 0.0
    const = np.full((2, 32, 48, 3), 77, np.uint8)
    with np.errstate(all="raise"):                      # no division by the zero deviation
        vals, mean = O.swd(const, const, 2, 5, dirs)
    assert vals == [0.0, 0.0] and mean == 0.0
    one = c["reals"].copy()
    one[..., 1] = 200                                   # one constant channel: its normalised values are zeros
    z = O.normalise(O.descriptors(O.pyramid(one, 2)[1], 1, 11, 19).astype(np.float32))
    assert not z.reshape(-1, 3, 49)[:, 1].any() and z.reshape(-1, 3, 49)[:, 0].any() and np.isfinite(z).all()
    vals, mean = O.swd(one, c["fakes"], 2, 11, dirs)
    assert np.isfinite(vals).all() and mean > 0
    # a different set scores above zero, and the score is symmetric
    v1, m1 = O.swd(c["fakes"], c["reals"], 2, 11, dirs)
    v2, m2 = O.swd(c["reals"], c["fakes"], 2, 11, dirs)
    assert m1 > 0 and v1 == v2


def test_eps64_fixture_is_the_measured_float64_error_of_the_statement():
    """eps64 = the worst float64-against-longdouble difference of the oracle over the inputs the GPU tests use (projections
    relative to sum_k |z_k d_k|, scores relative to the score).  The committed numbers are what the GPU bound of 16 * eps64
    multiplies.  The statement has its own summation order (no BLAS), so a re-measurement on another x87 host gives the same
    figures; the window of a factor of 4 either way is for a NumPy whose pairwise sums split differently."""
    g = O.golden_eps64()
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 here")
    now = O.measured_eps64()
    print("eps64 committed", g, "measured", now)
    for key in ("proj", "score"):
        assert g[key] / 4 <= now[key] <= g[key] * 4
        assert 2.0 ** -56 < g[key] < 1e-12          # of the size of float64 roundings, far from a float32 computation


# ------------------------------------------------------------------------------------------------ the C ABI
def _decl_params(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sggan.h")).read(), flags=re.S)
    decl = re.search(r"\b%s\((.*?)\);" % name, src, flags=re.S)
    assert decl, name + " not declared"
    return [p.split()[-1].lstrip("*") for p in decl.group(1).split(",")]


def test_entry_points_are_declared_and_bound():
    assert _decl_params("size_t sgg_swd_pyramid_elems") == ["H", "W", "levels"]
    assert _decl_params("size_t sgg_swd_pyramid_workspace") == ["N", "H", "W", "levels"]
    assert _decl_params("size_t sgg_swd_project_workspace") == ["M"]
    assert _decl_params("int sgg_swd_pyramid") == ["img", "kind", "cstride", "N", "H", "W", "levels", "pyr", "ws", "ws_bytes", "stream"]
    assert _decl_params("int sgg_swd_descriptors") == ["pyr", "N", "H", "W", "levels", "level", "patches", "seed", "image_offset", "desc", "stream"]
    assert _decl_params("int sgg_swd_project") == ["desc", "M", "dirs", "D", "proj", "moments", "ws", "ws_bytes", "stream"]
    assert _decl_params("int sgg_swd_distance") == ["sa", "sb", "D", "M", "out", "stream"]
    L = A.lib()
    for name in ("sgg_swd_pyramid_elems", "sgg_swd_pyramid_workspace", "sgg_swd_project_workspace", "sgg_swd_pyramid", "sgg_swd_descriptors",
                 "sgg_swd_project", "sgg_swd_distance"):
        assert name in A.SIGNATURES and hasattr(L, name)
        assert len(A.SIGNATURES[name][1]) == len(_decl_params(r"\w+ " + name))


def test_workspace_formulas():
    from sggan_amd import kernels as K
    L = A.lib()
    for H, W, lv in ((16, 16, 1), (32, 48, 2), (64, 96, 3), (112, 176, 5), (256, 512, 5), (2048, 2048, 5), (7, 7, 1)):
        elems = sum(3 * (H >> l) * (W >> l) for l in range(lv))
        assert L.sgg_swd_pyramid_elems(H, W, lv) == elems == K.swd_pyramid_elems(H, W, lv)
        assert L.sgg_swd_pyramid_workspace(3, H, W, lv) == 3 * elems * 8
    # unsupported shapes: 0
    for H, W, lv in ((16, 16, 0), (16, 16, 6), (30, 48, 3), (48, 30, 3), (48, 48, 4), (6, 64, 1), (4096, 2048, 1), (0, 16, 1), (16, -4, 1)):
        assert L.sgg_swd_pyramid_elems(H, W, lv) == 0 and L.sgg_swd_pyramid_workspace(1, H, W, lv) == 0, (H, W, lv)
    assert L.sgg_swd_pyramid_workspace(0, 16, 16, 1) == 0
    chunk = K.SWD_CHUNK
    for M in (1, 3, 33, chunk, chunk + 1, 768, 64000):
        assert L.sgg_swd_project_workspace(M) == 24 * ((M + chunk - 1) // chunk)
    assert L.sgg_swd_project_workspace(0) == 0 and L.sgg_swd_project_workspace(-5) == 0
    assert K.swd_default_levels(256, 512) == 5 and K.swd_default_levels(128, 128) == 4 and K.swd_default_levels(64, 64) == 3
    assert K.swd_default_levels(15, 64) == 0 and K.swd_default_levels(16, 16) == 1 and K.swd_default_levels(112, 176) == 3
    for H, W in ((256, 512), (128, 128), (64, 64), (16, 16), (48, 80)):
        assert K.swd_default_levels(H, W) == O.default_levels(H, W) and K.swd_pyramid_elems(H, W, K.swd_default_levels(H, W)) > 0


def test_every_refusal_comes_before_any_launch():
    """Bad arguments are answered on the host (the buffers are host memory that is never dereferenced; no call here is valid)."""
    L = A.lib()
    raw = (C.c_char * 512)()
    base = (C.addressof(raw) + 15) & ~15
    p, q, r = C.c_void_p(base), C.c_void_p(base + 64), C.c_void_p(base + 128)
    odd4, odd2, odd1 = C.c_void_p(base + 4), C.c_void_p(base + 2), C.c_void_p(base + 1)
    EI, EU, EW = A.EINVAL, A.EUNSUPPORTED, A.EWORKSPACE

    pyr = lambda img=p, kind=A.SGG_U8, cs=3, N=1, H=32, W=48, lv=2, out=q, ws=r, nbytes=1 << 40: \
        L.sgg_swd_pyramid(img, kind, cs, N, H, W, lv, out, ws, nbytes, None)
    need = L.sgg_swd_pyramid_workspace(1, 32, 48, 2)
    assert need == 8 * 3 * (32 * 48 + 16 * 24)
    assert pyr(nbytes=need - 1) == EW and pyr(nbytes=0) == EW
    assert pyr(img=None) == EI and pyr(out=None) == EI and pyr(ws=None) == EI
    assert pyr(out=odd2) == EI and pyr(ws=odd4) == EI                                   # float / double alignment
    assert pyr(kind=A.SGG_F32, cs=3, img=odd2) == EI and pyr(kind=A.SGG_BF16, cs=8, img=odd1) == EI
    assert pyr(kind=3) == EI and pyr(kind=-1) == EI
    assert pyr(cs=2) == EI and pyr(cs=5) == EI and pyr(kind=A.SGG_F32, cs=2) == EI and pyr(kind=A.SGG_BF16, cs=2) == EI
    assert pyr(N=0) == EI and pyr(N=-3) == EI
    assert pyr(lv=0) == EU and pyr(lv=6) == EU
    assert pyr(H=34, lv=3) == EU and pyr(W=50, lv=3) == EU                             # not divisible by 4
    assert pyr(H=48, W=48, lv=4) == EU and pyr(H=6, W=64, lv=1) == EU                   # coarsest 6x6 / 6x64
    assert pyr(H=4096, W=2048, lv=1) == EU                                              # H*W > 2^22
    assert pyr(N=21846) == EU                                                           # the grid: 3 N planes > 65535
    assert pyr(N=21845, nbytes=0) == EW
    assert pyr(kind=A.SGG_F32, cs=3, nbytes=0) == EW and pyr(kind=A.SGG_BF16, cs=8, nbytes=0) == EW and pyr(cs=4, nbytes=0) == EW

    desc = lambda pyr_=p, N=1, H=32, W=48, lv=2, level=0, patches=4, seed=19, off=0, out=q: \
        L.sgg_swd_descriptors(pyr_, N, H, W, lv, level, patches, seed, off, out, None)
    assert desc(pyr_=None) == EI and desc(out=None) == EI and desc(pyr_=odd2) == EI and desc(out=odd1) == EI
    assert desc(N=0) == EI and desc(patches=0) == EI and desc(patches=-1) == EI
    assert desc(level=2) == EI and desc(level=5) == EI and desc(level=-1) == EI
    assert desc(off=-1) == EI
    assert desc(lv=0) == EU and desc(lv=6, level=5) == EU and desc(H=34, lv=3) == EU and desc(H=6, W=64, lv=1) == EU
    assert desc(H=4096, W=2048, lv=1) == EU
    assert desc(N=65536) == EU and desc(patches=(1 << 31) // 147 + 1) == EU             # the grid

    proj = lambda d=p, M=33, dirs=q, D=128, out=r, mom=p, ws=q, nbytes=1 << 40: L.sgg_swd_project(d, M, dirs, D, out, mom, ws, nbytes, None)
    assert proj(nbytes=L.sgg_swd_project_workspace(33) - 1) == EW and proj(M=257, nbytes=24) == EW
    for hole in ("d", "dirs", "out", "mom", "ws"):
        assert proj(**{hole: None}) == EI, hole
    for arg, bad in (("d", odd2), ("dirs", odd1), ("out", odd4), ("mom", odd4), ("ws", odd4)):
        assert proj(**{arg: bad}) == EI, arg
    assert proj(M=0) == EI and proj(M=-1) == EI and proj(D=0) == EI and proj(D=-128) == EI
    assert proj(D=65535 * 128 + 1) == EU and proj(M=32 * (1 << 31)) == EU               # the grid

    dist = lambda a=p, b=q, D=128, M=33, out=r: L.sgg_swd_distance(a, b, D, M, out, None)
    assert dist(a=None) == EI and dist(b=None) == EI and dist(out=None) == EI
    assert dist(a=odd4) == EI and dist(b=odd4) == EI and dist(out=odd4) == EI
    assert dist(D=0) == EI and dist(M=0) == EI and dist(D=-1) == EI and dist(M=-1) == EI


def test_swd_kernels_do_not_spill(tmp_path):
    """csrc/swd.hip is in the build and recompiles with no spills and no scratch in every kernel."""
    sys.path.insert(0, os.path.join(ROOT, "sg-gan-tf2_amd"))
    import build as B
    assert "swd.hip" in B.SOURCES and "-ffp-contract=off" in B.FLAGS
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, *B.FLAGS, "-c", os.path.join(B.CSRC, "swd.hip"), "-o", str(tmp_path / "swd.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    pats = (("vspill", r"VGPRs Spill: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"))
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        for key, pat in pats:
            m = re.search(pat, line)
            if m and name:
                usage[name][key] = int(m.group(1))
    for frag, count in (("swd_quant_kernel", 1), ("swd_down_kernel", 1), ("swd_lap_kernel", 2), ("swd_descriptor_kernel", 1),
                        ("swd_sum_kernel", 2), ("swd_fold_kernel", 1), ("swd_project_kernel", 2), ("swd_distance_kernel", 1)):
        hits = [v for k, v in usage.items() if frag in k]
        assert len(hits) == count, f"kernel {frag}: {len(hits)} instances in the build"
        for h in hits:
            assert h == {"vspill": 0, "sspill": 0, "scratch": 0}, (frag, h)
    assert len(usage) == 11, sorted(usage)


# ------------------------------------------------------------------------------------------------ flags
def test_flags_are_absent_unless_given():
    from sggan_amd.main import build_parser, check_swd, parse_args
    a = parse_args(["--swd", "--swd_patches", "64"])
    assert a.swd is True and a.swd_patches == 64
    plain = vars(parse_args([]))
    assert "swd" not in plain and "swd_patches" not in plain and "swd_reals" not in plain
    assert not hasattr(parse_args(["--swd"]), "swd_patches") and not hasattr(parse_args(["--swd_patches", "3"]), "swd")
    text = " ".join(build_parser().format_help().split())
    for word in ("--swd", "--swd_patches", "SWD Mean", "--image_scores"):
        assert word in text, word
    check_swd(parse_args([]))                                   # off: nothing to check
    check_swd(parse_args(["--swd"]))                            # 64 x 64: three levels
    with pytest.raises(ValueError, match=r"min\(H, W\) >> \(L-1\) >= 16"):
        check_swd(parse_args(["--swd", "--img_height", "12", "--img_width", "64"]))
    with pytest.raises(ValueError):
        check_swd(parse_args(["--swd", "--swd_patches", "0"]))


def test_default_args_carry_the_switch_off():
    from sggan_amd.model import default_args
    d = default_args()
    assert d.swd is False and d.swd_patches == 128
    assert default_args(swd=True).swd is True
