"""Class-level evaluation without a GPU: the facts about the fixture that make a learned palette necessary and
sufficient, the oracle's own rules on hand-made cases, the C-ABI declarations, the argument checks the library answers from the
host, the register budget of csrc/evalseg.hip, and the flag surface."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from sggan_amd import _abi as A
from tests import class_scores_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sg-gan-tf2_amd"))

EXPORTS = {"sgg_palette_decode": 15, "sgg_palette_probs": 14, "sgg_class_boundary_band": 7}


# ---- the fixture -----------------------------------------------------------------------------------------------------------
def test_learned_palette_of_the_fixture_has_19_entries_and_the_known_colours():
    keys, classes = O.city_palette()
    assert keys.dtype == np.uint32 and classes.dtype == np.uint8 and len(keys) == len(classes) == 19
    table = dict(zip(keys.tolist(), classes.tolist()))
    assert table[0x804080] == 7 and table[0x464646] == 11 and table[0x999999] == 17
    assert table[0x000000] == 4                                # 37 308 px of id 4 against 37 px of id 0: the majority
    assert int(classes.max()) < 34
    # ordered by descending pixel count: re-count and compare
    count = {}
    for label, _ in O.city_pairs():
        rgb = label[..., :3].astype(np.int64)
        k, n = np.unique((rgb[..., 0] << 16) | (rgb[..., 1] << 8) | rgb[..., 2], return_counts=True)
        for kk, nn in zip(k.tolist(), n.tolist()):
            count[kk] = count.get(kk, 0) + nn
    assert set(count) == set(table)                            # every label pixel is one of 19 exact colours
    order = [(-count[k], k) for k in keys.tolist()]
    assert order == sorted(order)
    assert len(O.learn_palette(O.city_pairs(), max_entries=5)[0]) == 5 and np.array_equal(O.learn_palette(O.city_pairs(), 5)[0], keys[:5])


def test_learned_palette_redecodes_the_colour_labels_to_the_class_maps():
    """Measured: 100 %, 100 % and 99.993 % (the black pixels of id 0 in one file)."""
    keys, classes = O.city_palette()
    shares = []
    for label, classmap in O.city_pairs():
        got = O.labels(label, keys, classes)
        assert int(O.distances(O.colours(label), keys).min(axis=-1).max()) == 0          # exact colours only
        shares.append(float((got == classmap).mean()))
    print("agreement per file:", shares)
    assert all(s >= 0.9999 for s in shares) and sum(s == 1.0 for s in shares) == 2


def test_builtin_table_is_not_the_ground_truth_of_the_fixture():
    """Why the palette is learned: the 21-colour, 8-class table agrees with the class PNGs nowhere and misses colours."""
    from sggan_amd import segment_class as sc
    keys, classes = sc.palette()
    assert keys.dtype == np.uint32 and classes.dtype == np.uint8 and len(keys) == 21
    assert dict(zip(((int(k) >> 16, (int(k) >> 8) & 255, int(k) & 255) for k in keys), classes.tolist())) == dict(sc.cityscape())
    for label, classmap in O.city_pairs():
        d = O.distances(O.colours(label), keys).min(axis=-1)
        covered = float((d == 0).mean())
        exact = np.where(d == 0, O.labels(label, keys, classes), 0)
        print("covered", covered, "agree", float((exact == classmap).mean()))
        assert 0.85 <= covered <= 0.95 and float((exact == classmap).mean()) < 0.001


def test_package_learn_palette_equals_the_oracle_on_array_pairs():
    from sggan_amd import segment_class as sc
    pairs = O.city_pairs()
    keys, classes = sc.learn_palette(pairs)
    assert keys.dtype == np.uint32 and classes.dtype == np.uint8
    assert np.array_equal(keys, O.city_palette()[0]) and np.array_equal(classes, O.city_palette()[1])
    k3, c3 = sc.learn_palette(pairs, max_entries=3)
    assert np.array_equal(k3, keys[:3]) and np.array_equal(c3, classes[:3])
    # majority tie -> the lowest class; count tie -> the lower key first; alpha ignored
    label = np.zeros((2, 2, 4), dtype=np.uint8)
    label[0, :, 0] = 9
    label[..., 3] = [[1, 2], [3, 4]]
    kt, ct = sc.learn_palette([(label, np.array([[5, 3], [7, 7]], dtype=np.uint8))])
    assert kt.tolist() == [0x000000, 0x090000] and ct.tolist() == [7, 3]
    assert [a.tolist() for a in O.learn_palette([(label, np.array([[5, 3], [7, 7]], dtype=np.uint8))])] == [kt.tolist(), ct.tolist()]


# ---- the oracle's rules on cases worked by hand ------------------------------------------------------------------------------
def test_oracle_quantise_ties_threshold_band_and_probabilities_by_hand():
    x = np.array([[-1.0, 1.0, 0.0], [-1.0001, 1.0001, np.nan], [np.inf, -np.inf, 0.999], [-0.999, 0.5, -0.5]], dtype=np.float32)
    assert O.quantise(x).tolist() == [[0, 255, 127], [0, 255, 0], [255, 0, 254], [0, 191, 63]]
    from sggan_amd.utils import inverse_transform
    inside = np.linspace(-1, 1, 4099, dtype=np.float32).reshape(-1, 1).repeat(3, axis=1)
    assert np.array_equal(O.quantise(inside), inverse_transform(inside).astype(np.int64))          # utils.inverse_transform in [-1,1]
    keys, classes = np.array([0x0A0000, 0x0E0000, 0x0A0000], dtype=np.uint32), np.array([5, 6, 7], dtype=np.uint8)
    px = np.array([[[12, 0, 0], [10, 0, 0], [13, 0, 0], [10, 3, 0], [10, 3, 1]]], dtype=np.uint8)
    assert O.labels(px, keys, classes).tolist() == [[5, 5, 6, 5, 5]]                                # ties (d2 4|4, 0|0) to the lowest k
    assert O.labels(px, keys, classes, other_class=9, max_dist2=9).tolist() == [[5, 5, 6, 5, 9]]    # d2 = 9 kept, d2 = 10 -> other
    cls = np.zeros((1, 5, 6), dtype=np.uint8)
    cls[0, 0, 5] = 1
    assert not O.band(cls, 0).any()
    b1 = O.band(cls, 1)[0]
    assert b1.sum() == 4 and b1[0, 4] and b1[0, 5] and b1[1, 4] and b1[1, 5]
    assert O.band(cls, 8).all() and not O.band(np.zeros((1, 2, 3), dtype=np.uint8), 3).any()
    p = O.probs(px[None], keys[:2], classes[:2], 8, sigma=2.0)                                      # (1, 8, 1, 5)
    assert p.shape == (1, 8, 1, 5) and np.abs(p.sum(axis=1) - 1).max() < 1e-15
    assert np.array_equal(p[0, :, 0, 0] > 0, np.array([0, 0, 0, 0, 0, 1, 1, 0], dtype=bool)) and p[0, 5, 0, 0] == p[0, 6, 0, 0] == 0.5
    e = np.exp(-(16 - 0) / 8.0)
    assert abs(p[0, 6, 0, 1] - e / (1 + e)) < 1e-15
    po = O.probs(px[None], keys[:2], classes[:2], 8, sigma=2.0, other_class=0, max_dist2=1)         # a pseudo-distance for class 0
    assert po[0, 0, 0, 1] > 0 and abs(po[0, 0, 0, 1] - np.exp(-1 / 8.0) / (1 + np.exp(-1 / 8.0) + e)) < 1e-15
    h = O.hist([0, 1, 1, 9], [1, 1, 0, 0], 2, select=[1, 1, 0, 1])
    assert h.tolist() == [[0, 1], [0, 1]]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_exports_declared_in_header_abi_and_library():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sggan.h")).read(), flags=re.S)
    assert os.path.exists(A.LIB_PATH), "run `python __graft_entry__.py build` first"
    L = ctypes.CDLL(A.LIB_PATH)
    for name, nargs in EXPORTS.items():
        decl = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert name in A.SIGNATURES and len(A.SIGNATURES[name][1]) == nargs, name
        assert hasattr(L, name), f"{name} not exported by libsggan.so"
    assert A.SGG_U8 == 2 and re.search(r"SGG_U8\s*=\s*2", src)


def test_host_side_argument_checks_without_gpu():
    """Everything the three entry points refuse before they launch: answered from the host, no device needed."""
    L = A.lib()
    x = ctypes.c_void_p(4096)                                                        # never dereferenced by a refused call
    keys = (ctypes.c_uint32 * 65)(*([0x102030] * 65))
    cls = (ctypes.c_uint8 * 65)(*([5] * 65))

    def decode(img=x, kind=A.SGG_BF16, n=10, cs=8, k=keys, c=cls, K=19, other=0, md=-1, labels=x, truth=None, select=None, n_class=0, hist=None):
        return L.sgg_palette_decode(img, kind, n, cs, k, c, K, other, md, labels, truth, select, n_class, hist, None)
    assert decode(img=None) == A.EINVAL and decode(n=0) == A.EINVAL and decode(kind=3) == A.EINVAL
    assert decode(cs=2) == A.EINVAL and decode(kind=A.SGG_U8, cs=8) == A.EINVAL and decode(n=1 << 31) == A.EUNSUPPORTED
    assert decode(K=0) == A.EINVAL and decode(K=65) == A.EINVAL and decode(c=None) == A.EINVAL and decode(k=None) == A.EINVAL
    assert decode(other=256) == A.EINVAL and decode(other=-1) == A.EINVAL
    assert decode(labels=None) == A.EINVAL                                                          # no output at all
    assert decode(truth=x) == A.EINVAL and decode(hist=x, n_class=34) == A.EINVAL                   # truth and hist go together
    assert decode(select=x) == A.EINVAL
    assert decode(truth=x, hist=x, n_class=0) == A.EINVAL and decode(truth=x, hist=x, n_class=65) == A.EINVAL
    assert decode(truth=x, hist=x, n_class=5) == A.EINVAL                                           # n_class <= a palette class
    assert decode(k=None, c=None, K=0, truth=x, hist=x, n_class=7) == A.EINVAL                      # built-in table: classes up to 7
    bad = (ctypes.c_uint32 * 2)(0x102030, 0x1000000)
    assert decode(k=bad, K=2) == A.EINVAL                                                           # a key above 24 bits

    def probs(img=x, kind=A.SGG_F32, N=1, HW=10, cs=3, k=keys, c=cls, K=19, other=0, md=-1, n_class=34, sigma=32.0, out=x):
        return L.sgg_palette_probs(img, kind, N, HW, cs, k, c, K, other, md, n_class, sigma, out, None)
    assert probs(img=None) == A.EINVAL and probs(out=None) == A.EINVAL and probs(N=0) == A.EINVAL and probs(HW=0) == A.EINVAL
    assert probs(K=0) == A.EINVAL and probs(K=65) == A.EINVAL and probs(n_class=0) == A.EINVAL and probs(n_class=65) == A.EINVAL
    assert probs(n_class=5) == A.EINVAL and probs(sigma=0.0) == A.EINVAL and probs(sigma=float("nan")) == A.EINVAL
    assert probs(other=256) == A.EINVAL and probs(cs=2) == A.EINVAL and probs(kind=A.SGG_U8, cs=5) == A.EINVAL

    band = lambda c=x, b=x, N=1, H=4, W=4, r=1: L.sgg_class_boundary_band(c, b, N, H, W, r, None)
    assert band(c=None) == A.EINVAL and band(b=None) == A.EINVAL and band(r=-1) == A.EINVAL and band(r=9) == A.EINVAL
    assert band(N=0) == A.EINVAL and band(H=0) == A.EINVAL and band(W=0) == A.EINVAL


def test_evalseg_kernels_use_no_scratch_and_do_not_spill(tmp_path):
    import build as B
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    assert "evalseg.hip" in B.SOURCES
    r = subprocess.run([hipcc, *B.FLAGS, "-c", os.path.join(B.CSRC, "evalseg.hip"), "-o", str(tmp_path / "evalseg.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        for key, pat in (("vspill", r"VGPRs Spill: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                usage[name][key] = int(m.group(1))
    # decode: three input kinds, with and without the fused histogram; probabilities: three input kinds; the band
    assert sum("palette_decode_kernel" in k for k in usage) == 6 and sum("palette_probs_kernel" in k for k in usage) == 3
    assert sum("class_boundary_band_kernel" in k for k in usage) == 1 and len(usage) == 10, sorted(usage)
    for k, v in usage.items():
        assert (v["vspill"], v["sspill"], v["scratch"]) == (0, 0, 0), (k, v)
        assert v["lds"] <= 16384, (k, v)                                                           # n_class <= 64 -> 16 KB of counters


# ---- flags -------------------------------------------------------------------------------------------------------------------
def test_flags_are_absent_unless_given_and_parse_when_given():
    from sggan_amd.main import parse_args
    bare = parse_args([])
    assert not any(hasattr(bare, k) for k in ("class_scores", "boundary_px", "class_max_dist", "class_palette"))
    a = parse_args(["--class_scores", "--boundary_px", "5", "--class_max_dist", "12"])
    assert a.class_scores is True and a.boundary_px == 5 and a.class_max_dist == 12
    assert vars(parse_args(["--class_scores"])).keys() - vars(bare).keys() == {"class_scores"}


def test_missing_class_folder_and_palette_class_out_of_range_are_errors(tmp_path):
    from types import SimpleNamespace
    from sggan_amd import main as M
    (tmp_path / "testA").mkdir()
    with pytest.raises(FileNotFoundError, match="testA_seg_class"):
        M.class_test_cache(SimpleNamespace(class_scores=True, segment_class=34), str(tmp_path), "cpu")
    ok = SimpleNamespace(segment_class=34, class_palette=O.city_palette())
    M.check_class_palette(ok)
    with pytest.raises(ValueError, match="segment_class"):
        M.check_class_palette(SimpleNamespace(segment_class=17, class_palette=O.city_palette()))


def test_synthetic_test_samples_draw_the_mask_once_after_the_triple():
    from types import SimpleNamespace
    from sggan_amd.main import synthetic_test_samples
    base = dict(image_height=8, image_width=8, segment_class=34)
    plain = list(synthetic_test_samples(SimpleNamespace(**base))())
    crf = list(synthetic_test_samples(SimpleNamespace(crf=True, **base))())
    cs = list(synthetic_test_samples(SimpleNamespace(class_scores=True, **base))())
    both = list(synthetic_test_samples(SimpleNamespace(crf=True, class_scores=True, **base))())
    assert all(len(s) == 3 for s in plain) and all(len(s) == 4 for s in crf + cs + both)
    for a, b, c in zip(crf, cs, both):
        assert all(np.array_equal(u, v) and np.array_equal(u, w) for u, v, w in zip(a[1:], b[1:], c[1:]))
    assert np.array_equal(plain[0][1], cs[0][1]) and np.array_equal(plain[0][2], cs[0][2])
