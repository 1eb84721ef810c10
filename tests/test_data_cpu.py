"""Input pipeline, host side (no GPU): the band tables against the float64 oracle, the epoch protocol against a literal
restatement of the reference loop, the file rules on the fixture folder, the ABI entry, and the kernel's build resources."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import sggan_amd  # noqa: F401
from sggan_amd import _abi as A
from sggan_amd import data as D

from tests import resample_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "city_small")

# (H0, W0) -> (H, W): the Cityscapes geometry, the reference's 128x128 default, the GTA geometry (non-integer scales)
GEOMETRIES = [((1024, 2048), (256, 512)), ((1024, 2048), (128, 128)), ((1052, 1914), (256, 512))]


def test_oracle_statements_agree():
    """The filter-and-interpolate statement and the dense-matrix statement are the same operator."""
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (96, 200, 3), dtype=np.uint8)
    a = O.load_train(x, 24, 40)
    b = O.dense_apply(x, (96, 96, 24), (200, 96, 40))
    print("two oracle statements, max |diff|:", np.abs(a - b).max())
    assert np.abs(a - b).max() <= 1e-12
    assert np.abs(O.load_test(x, 24, 40) - O.dense_apply(x, (96, 24), (200, 40))).max() <= 1e-12


@pytest.mark.parametrize("src,dst", GEOMETRIES)
def test_band_tables_equal_the_oracle(src, dst):
    """The float64 band applied in NumPy equals the oracle to 1e-12 (the f32 storage of the weights is checked on its own:
    every row sums to 1 within 1e-6; its effect on pixels is bounded with the kernel's, in the GPU tests)."""
    (H0, W0), (H, W) = src, dst
    rng = np.random.default_rng(H0 + W)
    x = rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8)
    want = O.load_train(x, H, W)
    rows, cols = D.band_table64((H0, H0, H)), D.band_table64((W0, H0, W))
    got = D.apply_tables(x, rows, cols)
    err = np.abs(got - want).max()
    print(f"{src}->{dst}: taps rows {rows[0].shape[1]} cols {cols[0].shape[1]}, steps {rows[2]} {cols[2]}, max |err| {err:.3e}")
    assert got.shape == (H, W, 3) and err <= 1e-12
    for (w64, st, step), n_in in ((rows, H0), (cols, W0)):
        assert st.min() >= 0 and (st + w64.shape[1]).max() <= n_in and np.all(np.diff(st) >= 0) and step == np.diff(st).max()
    for sizes in ((H0, H0, H), (W0, H0, W)):
        w32, st, step = D.band_table(sizes)
        assert w32.dtype == np.float32 and st.dtype == np.int32
        assert np.abs(w32.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6
        assert np.array_equal(st, D.band_table64(sizes)[1])
    # the one-stage chain of load_test_data
    got = D.apply_tables(x, D.band_table64((H0, H)), D.band_table64((W0, W)))
    assert np.abs(got - O.load_test(x, H, W)).max() <= 1e-12


def test_identity_axis_and_refused_upscale():
    w, st, step = D.band_table64((37, 37))
    assert w.shape == (37, 1) and np.array_equal(w, np.ones((37, 1))) and np.array_equal(st, np.arange(37)) and step == 1
    x = np.random.default_rng(1).integers(0, 256, (37, 64, 3), dtype=np.uint8)
    got = D.apply_tables(x, D.band_table64((37, 37, 37)), D.band_table64((64, 37, 16)))
    assert np.abs(got - O.load_train(x, 37, 16)).max() <= 1e-12
    with pytest.raises(ValueError):
        D.band_table64((64, 65))
    with pytest.raises(ValueError):
        D.train_tables(200, 100, 64, 64)         # portrait source: the square stage would upscale the columns
    with pytest.raises(ValueError):
        D.test_tables(64, 64, 32, 128)


class _StubDomain:
    def __init__(self, n):
        self.cache = list(range(n))


@pytest.mark.parametrize("n_files,batch,train_size", [(10, 3, 10 ** 8), (10, 2, 7), (5, 1, 3), (4, 8, 100)])
def test_epoch_protocol_equals_the_reference_loop(n_files, batch, train_size):
    """File order, batch count under --train_size and flip draws, three epochs, against model.py:219-228 + utils.py:201
    restated literally and driven by an identically seeded RandomState."""
    from types import SimpleNamespace
    files = ["f%02d" % i for i in range(n_files)]
    want = O.epoch_protocol(files, 3, batch, train_size, np.random.RandomState(5))
    b = D.DirectoryBatches.__new__(D.DirectoryBatches)
    b.args = SimpleNamespace(batch_size=batch, train_size=train_size)
    b.rng = np.random.RandomState(5)
    b.domains = [_StubDomain(n_files)]
    for ep in want:
        (order,), flips, n = b.epoch_plan()
        assert n == len(ep) == min(n_files, train_size) // batch
        got = [[(files[order[k * batch + i]], bool(flips[k * batch + i])) for i in range(batch)] for k in range(n)]
        assert got == ep


def test_fixture_files_siblings_and_grouping():
    """Sorted listing, the reference's ``.replace`` sibling rule, PIL decoding and grouping by source shape (host tensors)."""
    c = D.DatasetCache(FIX, "trainA", device="cpu")
    assert [os.path.basename(f) for f in c.files] == ["aachen_000000.png", "aachen_000001.png"] and len(c) == 2
    assert c.seg_files[0] == os.path.join(FIX, "trainA_seg", "aachen_000000.png")
    assert c.class_files[1] == os.path.join(FIX, "trainA_seg_class", "aachen_000001.png")
    assert D.sibling("./datasets/city/trainA/x.png", "trainA", "_seg_class") == "./datasets/city/trainA_seg_class/x.png"
    assert set(c.stacks) == {("image", 512, 1024, 3), ("label", 512, 1024, 4), ("class", 512, 1024)}
    assert c.image == [(("image", 512, 1024, 3), 0), (("image", 512, 1024, 3), 1)]
    from PIL import Image
    for where, paths in ((c.image, c.files), (c.label, c.seg_files), (c.classmap, c.class_files)):
        for (key, i), p in zip(where, paths):
            assert np.array_equal(c.stacks[key][i].numpy(), np.asarray(Image.open(p)))
    assert len(D.DatasetCache(FIX, "trainA", device="cpu", max_files=1)) == 1
    t = D.DatasetCache(FIX, "testA", device="cpu", with_class=False)
    assert t.classmap is None and os.path.basename(t.seg_files[0]) == "aachen_000016.png"
    assert D.resolve_root(FIX) == FIX and D.resolve_root(os.path.join(FIX, "nothing_here")) is None
    with pytest.raises(FileNotFoundError):
        D.DatasetCache(FIX, "trainB", device="cpu")


def test_mixed_source_shapes_are_grouped(tmp_path):
    """A folder whose files differ in size (the GTA folder's 1914x1052 beside 2048x1024) and a palette label."""
    from PIL import Image
    rng = np.random.default_rng(3)
    for sub in ("trainA", "trainA_seg", "trainA_seg_class"):
        os.makedirs(tmp_path / sub)
    for name, (h, w) in (("a", (20, 40)), ("b", (24, 36)), ("c", (20, 40))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / "trainA" / f"{name}.png")
        pal = Image.fromarray(rng.integers(0, 4, (h, w), dtype=np.uint8), mode="P")
        pal.putpalette([0, 0, 0, 128, 64, 128, 244, 35, 232, 70, 70, 70] + [0] * (252 * 3))
        pal.save(tmp_path / "trainA_seg" / f"{name}.png")
        Image.fromarray(rng.integers(0, 34, (h, w), dtype=np.uint8)).save(tmp_path / "trainA_seg_class" / f"{name}.png")
    c = D.DatasetCache(str(tmp_path), "trainA", device="cpu")
    assert c.image == [(("image", 20, 40, 3), 0), (("image", 24, 36, 3), 0), (("image", 20, 40, 3), 1)]
    assert c.label[1] == (("label", 24, 36, 3), 0)                 # palette label -> RGB
    assert tuple(c.stacks[("image", 20, 40, 3)].shape) == (2, 20, 40, 3) and tuple(c.stacks[("class", 24, 36)].shape) == (1, 24, 36)
    exp = np.asarray(Image.open(tmp_path / "trainA_seg" / "b.png").convert("RGB"))
    assert np.array_equal(c.stacks[("label", 24, 36, 3)][0].numpy(), exp)


def test_resample_symbol_is_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sggan.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+sgg_resample_u8\s*\(", hdr)
    assert "sgg_resample_u8" in A.SIGNATURES and len(A.SIGNATURES["sgg_resample_u8"][1]) == 21
    assert hasattr(ctypes.CDLL(A.LIB_PATH), "sgg_resample_u8")
    from sggan_amd import kernels as K
    assert callable(K.resample_u8)
    # argument validation happens before anything touches a device
    f = A.lib().sgg_resample_u8
    p = ctypes.c_void_p(64)
    ok = [p, 1, 8, 8, 3, p, p, p, p, 1, p, p, 1, 1, p, 1, 8, 8, 3, A.SGG_F32, None]
    for pos, bad in ((0, None), (4, 5), (18, 4), (9, 9), (12, 0), (19, 7), (14, ctypes.c_void_p(68))):
        args = list(ok)
        args[pos] = bad
        assert f(*args) == A.EINVAL, pos


def test_resample_kernel_build_resources(tmp_path):
    """csrc/resample.hip recompiled with -Rpass-analysis=kernel-resource-usage (the method of tests/test_build_resources.py):
    every instantiation of the kernel has zero VGPR spills and uses no scratch."""
    sys.path.insert(0, os.path.join(ROOT, "sg-gan-tf2_amd"))
    import build as B
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    assert "resample.hip" in B.SOURCES
    r = subprocess.run([hipcc, *B.FLAGS, "-c", os.path.join(B.CSRC, "resample.hip"), "-o", str(tmp_path / "resample.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        for key, pat in (("spill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vgprs", r" VGPRs: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                usage[name][key] = int(m.group(1))
    hits = {k: v for k, v in usage.items() if "resample_u8_kernel" in k}
    assert len(hits) == 4, sorted(usage)                       # Cs 3 / 4 x bf16 / f32
    for k, v in hits.items():
        print(k, v)
        assert v.get("spill") == 0 and v.get("scratch") == 0, (k, v)
