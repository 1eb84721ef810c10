"""CPU-side checks of the discriminators' differentiable augmentation (--diffaug): the generator's known answers,
the NumPy statement's own adjoint identity, the parameter rows' ranges and policy switches, the flags, the C ABI of the four
entry points (host-side validation only: no GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sggan_amd import _abi as A
from tests import diffaug_oracle as DO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox4x32_10_known_answers():
    """Random123's known-answer vectors for philox4x32 with 10 rounds."""
    kat = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for ctr, key, want in kat:
        assert DO.philox4x32_10(ctr, key) == want, [hex(w) for w in DO.philox4x32_10(ctr, key)]


def _rows(kind, H, W, rng):
    if kind == "neutral":
        return np.tile(DO.NEUTRAL, (2, 1))
    if kind == "random":
        return np.concatenate([DO.param_rows(t, 19, 5, 1, sid, H, W, DO.COLOR | DO.CUTOUT) for t, sid in ((0, 0), (7, 3))])
    p = DO.param_rows(3, 19, 0, 2, 1, H, W, DO.COLOR | DO.CUTOUT)
    ch, cw = H // 2, W // 2
    if kind == "no_cutout":
        p[:, 3:7] = 0
    else:                                       # a rectangle that sticks out over one border
        p[:, 3] = {"top": -(ch // 2), "bottom": H - ch // 2}.get(kind, 2)
        p[:, 4] = {"left": -(cw // 2), "right": W - cw // 2}.get(kind, 3)
    return p


@pytest.mark.parametrize("kind", ["random", "neutral", "top", "bottom", "left", "right", "no_cutout"])
def test_adjoint_identity_of_the_numpy_statement(kind):
    """T is affine in x for fixed rows: <T(x1) - T(x0), g> == <x1 - x0, T^T g> to 1e-12 relative."""
    rng = np.random.default_rng(5)
    H, W, Cn = 11, 13, 3
    p = _rows(kind, H, W, rng)
    x0, x1, g = (rng.uniform(-1, 2, (2, H, W, Cn)) for _ in range(3))
    lhs = float(((DO.forward(x1, p) - DO.forward(x0, p)) * g).sum())
    rhs = float(((x1 - x0) * DO.adjoint(g, p)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    if kind == "neutral":
        assert np.array_equal(DO.forward(x0, p), x0) and np.array_equal(DO.adjoint(g, p), g)
    elif kind != "no_cutout":                   # the clipped rectangle is there, and smaller than the whole one
        holes = (DO.forward(x0 + 10.0, p) == 0).all(-1).sum(axis=(1, 2))
        full = (H // 2) * (W // 2)
        assert np.all(holes > 0) and (np.all(holes < full) if kind != "random" else np.all(holes <= full)), holes
    else:
        assert not (DO.forward(x0 + 10.0, p) == 0).any()
    a = rng.uniform(-1, 1, g.shape)
    assert np.array_equal(DO.adjoint(g, p, addend=a), DO.adjoint(g, p) + a)


def test_parameter_rows_ranges_and_policy_switches():
    H, W, B = 11, 14, 0.25
    both = np.concatenate([DO.param_rows(t, 19, 0, 64, sid, H, W, DO.COLOR | DO.CUTOUT, B) for t in (0, 1, (1 << 32) + 5) for sid in (0, 1)])
    b, s, c, y0, x0, ch, cw, z = both.T
    assert both.dtype == np.float32 and np.all(z == 0)
    assert np.all(np.abs(b) <= B / 2) and np.all((s >= 0) & (s < 2)) and np.all((c >= 0.5) & (c <= 1.5))
    assert b.std() > 0.03 and s.std() > 0.3 and c.std() > 0.15                                  # (uniform: B/sqrt(12), 2/sqrt(12), 1/sqrt(12))
    assert np.all(ch == H // 2) and np.all(cw == W // 2)
    # floor(u * (H + 1 - ch % 2)) lies in 0 .. H - ch % 2; the rectangle starts ch // 2 in front of it
    assert np.all((y0 >= -2) & (y0 <= 11 - 1 - 2)) and np.all(y0 == np.floor(y0))                # H = 11: ch = 5
    assert np.all((x0 >= -3) & (x0 <= 14 - 1 - 3)) and np.all(x0 == np.floor(x0))                # W = 14: cw = 7
    assert len(np.unique(y0)) > 5 and len(np.unique(x0)) > 5
    colour = DO.param_rows(1, 19, 0, 8, 0, H, W, DO.COLOR, B)
    cut = DO.param_rows(1, 19, 0, 8, 0, H, W, DO.CUTOUT, B)
    first = DO.param_rows(1, 19, 0, 8, 0, H, W, DO.COLOR | DO.CUTOUT, B)
    assert np.array_equal(colour[:, :3], first[:, :3]) and not colour[:, 3:].any()
    assert np.array_equal(cut[:, 3:], first[:, 3:]) and np.array_equal(cut[:, :3], np.tile(DO.NEUTRAL[:3], (8, 1)))
    assert np.array_equal(DO.param_rows(1, 19, 0, 8, 0, H, W, 0, B), np.tile(DO.NEUTRAL, (8, 1)))
    # keyed by the sample, not by the row: one batch of 4 == two batches of 2 at offsets 0 and 2; streams and steps differ
    whole = DO.param_rows(9, 19, 0, 4, 2, H, W, 3, B)
    assert np.array_equal(whole, np.concatenate([DO.param_rows(9, 19, 0, 2, 2, H, W, 3, B), DO.param_rows(9, 19, 2, 2, 2, H, W, 3, B)]))
    assert not np.array_equal(whole, DO.param_rows(9, 19, 0, 4, 3, H, W, 3, B)) and not np.array_equal(whole, DO.param_rows(10, 19, 0, 4, 2, H, W, 3, B))
    assert not np.array_equal(whole, DO.param_rows(9, 20, 0, 4, 2, H, W, 3, B))


def test_policy_words_and_constructor_arguments():
    from sggan_amd import kernels as K
    from sggan_amd.model import default_args
    assert K.diffaug_policy_bits("color,cutout") == 3 and K.diffaug_policy_bits("cutout, color") == 3
    assert K.diffaug_policy_bits("color") == K.DIFFAUG_COLOR == DO.COLOR and K.diffaug_policy_bits("cutout") == K.DIFFAUG_CUTOUT == DO.CUTOUT
    assert K.diffaug_policy_bits(None) == 0 and K.diffaug_policy_bits("") == 0
    with pytest.raises(ValueError):
        K.diffaug_policy_bits("translation")
    d = default_args()
    assert d.diffaug is None and d.diffaug_brightness == 0.25
    assert default_args(diffaug="color").diffaug == "color"


def test_flags_are_absent_unless_given():
    from sggan_amd.main import build_parser, parse_args
    a = parse_args(["--diffaug", "color,cutout", "--diffaug_brightness", "0.5"])
    assert a.diffaug == "color,cutout" and a.diffaug_brightness == 0.5
    plain = vars(parse_args([]))
    assert "diffaug" not in plain and "diffaug_brightness" not in plain
    assert not hasattr(parse_args(["--diffaug", "color"]), "diffaug_brightness")
    text = " ".join(build_parser().format_help().split())
    for word in ("--diffaug POLICY", "--diffaug_brightness", "color,cutout", "--use_pool"):
        assert word in text, word


def test_entry_points_are_declared_bound_and_validate_on_the_host():
    """The four symbols with their documented argument lists, bound with matching ctypes; the workspace is one double per 2048-pixel
    chunk and row; bad arguments are refused before any launch (the buffers are host memory that is never dereferenced)."""
    from sggan_amd import kernels as K
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sggan.h")).read(), flags=re.S)
    def params(name):
        decl = re.search(r"\b%s\((.*?)\);" % name, src, flags=re.S)
        assert decl, name + " not declared"
        return [p.split()[-1] for p in decl.group(1).split(",")]
    assert params("size_t sgg_diffaug_workspace") == ["rows", "H", "W"]
    assert params("int sgg_diffaug_draw") == ["params", "rows", "iterations", "seed", "sample_offset", "stream_id", "H", "W", "policy_bits",
                                              "brightness", "stream"]
    assert params("int sgg_diffaug_fwd") == ["x", "y", "params", "rows", "H", "W", "C_real", "Cpad", "dtype", "ws", "ws_bytes", "stream"]
    assert params("int sgg_diffaug_bwd") == ["dy", "params", "addend", "dx", "rows", "H", "W", "C_real", "Cpad", "dtype", "ws", "ws_bytes",
                                             "stream"]
    for name in ("sgg_diffaug_workspace", "sgg_diffaug_draw", "sgg_diffaug_fwd", "sgg_diffaug_bwd"):
        assert name in A.SIGNATURES
    L = A.lib()
    chunk = K.DIFFAUG_CHUNK
    for rows, H, W in ((1, 1, 1), (3, 11, 13), (1, 32, 64), (2, 1, chunk + 1), (8, 256, 512)):
        assert L.sgg_diffaug_workspace(rows, H, W) == 8 * rows * ((H * W + chunk - 1) // chunk)
    assert L.sgg_diffaug_workspace(0, 4, 4) == 0 and L.sgg_diffaug_workspace(1, 0, 4) == 0 and L.sgg_diffaug_workspace(1, 1 << 14, 1 << 13) == 0

    raw = (C.c_char * 256)()
    base = (C.addressof(raw) + 15) & ~15
    p, q, odd = C.c_void_p(base), C.c_void_p(base + 64), C.c_void_p(base + 4)
    need = L.sgg_diffaug_workspace(2, 64, 128)
    ok = (2, 64, 128, 3, 8, A.SGG_BF16)
    assert L.sgg_diffaug_fwd(p, q, p, *ok, p, need - 1, None) == A.EWORKSPACE
    assert L.sgg_diffaug_bwd(p, p, None, q, *ok, p, need - 1, None) == A.EWORKSPACE
    assert L.sgg_diffaug_fwd(p, p, p, *ok, p, need, None) == A.EINVAL                                  # forward is out of place
    for hole in range(4):                                   # x, y, params, ws missing in turn
        a = [p, q, p, p]
        a[hole] = None
        assert L.sgg_diffaug_fwd(a[0], a[1], a[2], *ok, a[3], need, None) == A.EINVAL, hole
        assert L.sgg_diffaug_bwd(a[0], a[2], None, a[1], *ok, a[3], need, None) == A.EINVAL, hole
    assert L.sgg_diffaug_fwd(odd, q, p, *ok, p, need, None) == A.EINVAL and L.sgg_diffaug_bwd(p, p, odd, q, *ok, p, need, None) == A.EINVAL
    assert L.sgg_diffaug_fwd(p, q, p, 0, 64, 128, 3, 8, 1, p, need, None) == A.EINVAL
    assert L.sgg_diffaug_fwd(p, q, p, 2, 64, 128, 9, 8, 1, p, need, None) == A.EINVAL                  # C_real > Cpad
    assert L.sgg_diffaug_fwd(p, q, p, 2, 64, 128, 3, 8, A.SGG_U8, p, need, None) == A.EINVAL
    assert L.sgg_diffaug_fwd(p, q, p, 2, 64, 128, 3, 16, 1, p, need, None) == A.EUNSUPPORTED
    # a launch holds fewer than 2^32 threads, 256 per block: 2^24 blocks (8192 chunks x 2048 rows) are refused, one row less is not
    assert L.sgg_diffaug_fwd(p, q, p, 2048, 4096, 4096, 3, 8, 1, p, 1 << 40, None) == A.EUNSUPPORTED
    assert L.sgg_diffaug_bwd(p, p, None, q, 2048, 4096, 4096, 3, 8, 1, p, 1 << 40, None) == A.EUNSUPPORTED
    assert L.sgg_diffaug_fwd(p, q, p, 2047, 4096, 4096, 3, 8, 1, p, 0, None) == A.EWORKSPACE
    draw = lambda *a: L.sgg_diffaug_draw(*a, None)
    assert draw(None, 2, p, 19, 0, 0, 8, 8, 3, 0.25) == A.EINVAL and draw(p, 2, None, 19, 0, 0, 8, 8, 3, 0.25) == A.EINVAL
    assert draw(p, 0, p, 19, 0, 0, 8, 8, 3, 0.25) == A.EINVAL and draw(p, 2, p, 19, 0, -1, 8, 8, 3, 0.25) == A.EINVAL
    assert draw(p, 2, p, 19, 0, 0, 8, 8, 4, 0.25) == A.EINVAL and draw(p, 2, p, 19, -1, 0, 8, 8, 3, 0.25) == A.EINVAL
    assert draw(odd, 2, p, 19, 0, 0, 8, 8, 3, 0.25) == A.EINVAL


def test_diffaug_kernels_do_not_spill(tmp_path):
    """csrc/diffaug.hip recompiled with -Rpass-analysis=kernel-resource-usage (the method of tests/test_build_resources.py): the
    bandwidth kernels are in the build with no spills and no scratch, at full occupancy (they hide HBM latency with resident
    blocks)."""
    import shutil
    import subprocess
    import sys
    sys.path.insert(0, os.path.join(ROOT, "sg-gan-tf2_amd"))
    import build as B
    assert "diffaug.hip" in B.SOURCES
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, *B.FLAGS, "-c", os.path.join(B.CSRC, "diffaug.hip"), "-o", str(tmp_path / "diffaug.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    pats = (("vspill", r"VGPRs Spill: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
            ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"))
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
    for frag, count in (("diffaug_sum_kernel", 4), ("diffaug_fwd_kernel", 2), ("diffaug_bwd_kernel", 2), ("diffaug_draw_kernel", 1)):
        hits = [v for k, v in usage.items() if frag in k]
        assert len(hits) == count, f"kernel {frag}: {len(hits)} instances in the build"
        for h in hits:
            assert h == {"vspill": 0, "sspill": 0, "scratch": 0, "occ": 8}, (frag, h)
