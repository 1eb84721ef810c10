"""Input pipeline on the GPU: sgg_resample_u8 against the float64 oracle (tests/resample_oracle.py), the fixture folder end
to end through DirectoryBatches, graph replay fed in place, and the command line on a dataset directory.

Bounds.  f32 output: |err| <= 1e-5 -- each pass is a dot product of at most 64 non-negative weights summing to 1 with values
in [0, 1], error <= n * 2^-24 per pass, the tables' f32 rounding below that.  bf16 output: bit-equal to the f32 output rounded
to nearest-even, hence <= 2^-9 + 1e-5 from the oracle.  Every case is compared in full."""
import os

import numpy as np
import pytest
import torch

import sggan_amd as sg
from sggan_amd import data as D
from sggan_amd import kernels as K
from tests import resample_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "city_small")
DEV = "cuda:0"
F32_TOL, BF16_TOL = 1e-5, 2.0 ** -9 + 1e-5

# (H0, W0) -> (H, W): the three geometries of the issue at a quarter of the source size (same per-stage scales: 4 and 2 x 2;
# 8 and 2 x 8; 4.109 and 1.82 x 2.05), and the full Cityscapes case
CASES = [((256, 512), (64, 128)), ((256, 512), (32, 32)), ((263, 479), (64, 128)), ((1024, 2048), (256, 512))]


def _run(src, index, flip, tables, H, W, dtype, C=3):
    rows, cols = D._device_tables(tables, DEV)
    out = torch.full((len(index), H, W, 8), float("nan"), dtype=dtype, device=DEV)
    K.resample_u8(torch.as_tensor(src).to(DEV), torch.as_tensor(np.asarray(index, dtype=np.int32)).to(DEV),
                  torch.as_tensor(np.asarray(flip, dtype=np.int32)).to(DEV), rows, cols, out, C)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("Cs", [3, 4])
@pytest.mark.parametrize("src_hw,dst_hw", CASES)
def test_resample_u8_against_the_oracle(src_hw, dst_hw, Cs):
    (H0, W0), (H, W) = src_hw, dst_hw
    full = H0 >= 1024
    M = 2 if full else 3
    index, flip = ([1, 0, 1], [1, 0, 0]) if full else ([2, 0, 2, 1, 0], [0, 1, 1, 0, 0])     # repeated, out of order
    rng = np.random.default_rng(H0 * 7 + W + Cs)
    src = rng.integers(0, 256, (M, H0, W0, Cs), dtype=np.uint8)
    src[0, :4, :4] = 255; src[0, -4:, -4:] = 0; src[M - 1, :3] = 255                         # saturated borders
    want_src = [O.load_train(s, H, W)[..., :3] for s in src]
    want = np.stack([w[:, ::-1] if f else w for w, f in ((want_src[i], f) for i, f in zip(index, flip))])
    tables = D.train_tables(H0, W0, H, W)
    out32 = _run(src, index, flip, tables, H, W, torch.float32)
    out16 = _run(src, index, flip, tables, H, W, torch.bfloat16)
    got = out32.cpu().numpy().astype(np.float64)
    e32 = np.abs(got[..., :3] - want).max()
    e16 = np.abs(out16[..., :3].float().cpu().numpy().astype(np.float64) - want).max()
    print(f"{src_hw}->{dst_hw} Cs={Cs}: taps {tables[0][0].shape[1]}x{tables[1][0].shape[1]}  f32 max|err| {e32:.3e}  bf16 max|err| {e16:.3e}")
    assert e32 <= F32_TOL
    assert torch.equal(out16, out32.to(torch.bfloat16))                    # bf16 = RNE of the f32 result, bit for bit
    assert e16 <= BF16_TOL
    assert torch.count_nonzero(out32[..., 3:]) == 0 and torch.count_nonzero(out16[..., 3:]) == 0   # pad channels exactly zero
    assert not torch.isnan(out32).any()


def test_one_stage_tables_and_channel_count():
    """load_test_data's single resize, and C < 3 / C = 4 channel selections."""
    rng = np.random.default_rng(11)
    src = rng.integers(0, 256, (1, 200, 300, 4), dtype=np.uint8)
    want = O.load_test(src[0], 50, 100)
    t = D.test_tables(200, 300, 50, 100)
    for C in (1, 3, 4):
        out = _run(src, [0], [0], t, 50, 100, torch.float32, C=C)
        assert np.abs(out[0, ..., :C].cpu().numpy() - want[..., :C]).max() <= F32_TOL
        assert torch.count_nonzero(out[..., C:]) == 0


def test_flip_and_batch_position_are_bit_exact():
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, (3, 263, 479, 3), dtype=np.uint8)
    t = D.train_tables(263, 479, 64, 128)
    for dtype in (torch.float32, torch.bfloat16):
        a = _run(src, [0, 1, 2, 1, 1], [0, 0, 0, 1, 0], t, 64, 128, dtype)
        b = _run(src, [1, 1, 0, 2, 1, 0, 1], [1, 0, 1, 1, 0, 0, 1], t, 64, 128, dtype)
        assert torch.equal(a[3], a[1].flip(1))                             # flipped = unflipped reversed along W
        assert torch.equal(a[4], a[1]) and torch.equal(b[1], a[1]) and torch.equal(b[4], a[1]) and torch.equal(b[5], a[0])
        assert torch.equal(b[0], a[3]) and torch.equal(b[6], a[3]) and torch.equal(b[2], a[0].flip(1)) and torch.equal(b[3], a[2].flip(1))
        wide = _run(src, [1], [0], D.train_tables(263, 479, 64, 263), 64, 263, dtype)   # two column tiles, a ragged one
        ref = O.load_train(src[1], 64, 263)
        assert np.abs(wide[0, ..., :3].float().cpu().numpy() - ref).max() <= (F32_TOL if dtype == torch.float32 else BF16_TOL)


def _small_args(**kw):
    a = dict(ngf=8, ndf=8, n_blocks=2, batch_size=2, image_height=128, image_width=256, device=DEV, epoch=2, train_size=10 ** 8,
             checkpoint_dir=None, continue_train=False)
    a.update(kw)
    return sg.default_args(**a)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_directory_batches_on_the_fixture(dtype):
    """real_A / seg_A within the kernel bounds of the oracle applied to the PIL-decoded files, mask_A bit-equal to
    one_hot_mask of the class PNG, flipped where drawn; the yielded tensors are the same objects every step."""
    from PIL import Image
    from sggan_amd.segment_class import one_hot_mask
    args = _small_args(dtype=dtype, batch_size=1)
    model = sg.sggan(args)
    cache = D.DatasetCache(FIX, "trainA", device=DEV)
    batches = D.DirectoryBatches(model, args, cache, rng=np.random.RandomState(3))
    want = O.epoch_protocol(cache.files, 3, 1, args.train_size, np.random.RandomState(3))
    H, W = args.image_height, args.image_width
    mh, mw = D.mask_grid(model, H, W)
    tol = F32_TOL if dtype == "f32" else BF16_TOL
    seen, flips_seen = None, set()
    for ep, ep_want in enumerate(want):
        it = batches(ep)
        assert len(it) == len(ep_want) == 2
        for b, exp in zip(it, ep_want):
            ids = {k: id(v) for k, v in b.items()}
            assert seen is None or ids == seen
            seen = ids
            (path, flip), = exp
            flips_seen.add(bool(flip))
            img = np.asarray(Image.open(path)); lab = np.asarray(Image.open(D.sibling(path, "trainA", "_seg")))
            cls = np.asarray(Image.open(D.sibling(path, "trainA", "_seg_class")))
            for name, u8 in (("real_A", img), ("seg_A", lab)):
                ref = O.load_train(u8, H, W)[..., :3]
                ref = ref[:, ::-1] if flip else ref
                got = b[name]
                assert got.dtype == model.dtype and tuple(got.shape) == (1, H, W, 8)
                err = np.abs(got[0, ..., :3].float().cpu().numpy() - ref).max()
                print(f"{dtype} {os.path.basename(path)} {name} flip={flip}: max|err| {err:.3e}")
                assert err <= tol and torch.count_nonzero(got[..., 3:]) == 0
            m = one_hot_mask(cls, mh, mw, args.segment_class)
            assert torch.equal(b["mask_A"], m.flip(2) if flip else m)
    assert flips_seen == {True, False}            # (seed 3 draws both within the three epochs)


def _train(graph, cycle=False):
    args = _small_args(dtype="bf16", batch_size=1, graph=graph, cycle=cycle)
    model = sg.sggan(args)
    records = []
    rec = model._record
    model._record = lambda: (records.append(1), rec())[1]
    cache = D.DatasetCache(FIX, "trainA", device=DEV)
    batches = D.DirectoryBatches(model, args, cache, cache if cycle else None, rng=np.random.RandomState(3))   # (draws flips of both kinds)
    hist = model.train(args, batches, log=lambda s: None)
    torch.cuda.synchronize()
    return model, hist, len(records), batches


@pytest.mark.parametrize("cycle", [False, True])
def test_graph_replay_reads_the_loader_buffers_in_place(cycle):
    """Two epochs over the fixture: the graph run records the step once, adopts the loader's tensors as its static inputs
    (no staging copy) and ends with parameters bit-equal to the eager run's."""
    eager, h0, n0, _ = _train(False, cycle)
    graph, h1, n1, batches = _train(True, cycle)
    assert n0 == 0 and n1 == 1
    for k, v in batches.batch.items():
        assert graph._static_in[k] is v and getattr(graph, k) is v
    assert len(h1) == 2 and all(np.isfinite(h["Generator Loss"]) and np.isfinite(h["Discriminator Loss"]) for h in h0 + h1)
    for a, b in zip(eager.networks(), graph.networks()):
        assert torch.isfinite(b.P.flat).all() and torch.equal(a.P.flat, b.P.flat)
    assert [h["Generator Loss"] for h in h0] == [h["Generator Loss"] for h in h1]


def test_adopt_inputs_refuses_foreign_layouts():
    model = sg.sggan(_small_args(dtype="bf16"))
    with pytest.raises(ValueError):
        model.adopt_inputs(real_A=torch.zeros((2, 128, 256, 3), device=DEV))
    with pytest.raises(KeyError):
        model.adopt_inputs(real_B=torch.zeros((2, 128, 256, 8), dtype=torch.bfloat16, device=DEV))


def test_directory_test_samples_on_the_fixture():
    from PIL import Image
    args = _small_args()
    cache = D.DatasetCache(FIX, "testA", device=DEV, with_class=False)
    (name, img, seg), = list(D.directory_test_samples(args, cache)())
    assert name == "aachen_000016.png" and img.shape == seg.shape == (128, 256, 3) and img.dtype == np.float32
    for got, sub in ((img, "testA"), (seg, "testA_seg")):
        u8 = np.asarray(Image.open(os.path.join(FIX, sub, name)))
        assert np.abs(got - O.load_test(u8, 128, 256)[..., :3]).max() <= F32_TOL


def test_command_line_on_a_dataset_directory(tmp_path):
    """--dataset_dir <folder with trainA>: reference mode, --cycle (domain B via --dataset_dir_B) and --phase test run on the
    files and write the reference-named outputs; a name without a trainA folder keeps the synthetic sources."""
    from sggan_amd.main import main
    common = ["--img_height", "128", "--img_width", "256", "--ngf", "8", "--ndf", "8", "--epoch", "1", "--dataset_dir", FIX,
              "--log_dir", str(tmp_path / "logs")]
    hist = main(common + ["--checkpoint_dir", str(tmp_path / "ck"), "--test_dir", str(tmp_path / "test")])
    assert len(hist) == 1 and np.isfinite(hist[0]["Generator Loss"])
    assert os.path.exists(tmp_path / "ck" / "city_small" / "gen" / "cp-0000.ckpt") and os.path.exists(tmp_path / "ck" / "city_small" / "disc" / "cp-0000.ckpt")
    assert os.path.exists(tmp_path / "test" / "aachen_000016.png")           # the epoch-end test pass (model.py:362-365)
    hist = main(common + ["--cycle", "--graph", "--dataset_dir_B", FIX, "--checkpoint_dir", str(tmp_path / "ck2"), "--test_dir", str(tmp_path / "test2")])
    assert len(hist) == 1 and np.isfinite(hist[0]["Generator Loss"]) and np.isfinite(hist[0]["Discriminator Loss"])
    with pytest.raises(FileNotFoundError):
        main(common + ["--cycle", "--checkpoint_dir", str(tmp_path / "ck4")])     # the fixture has no trainB
    out = main(common + ["--phase", "test", "--checkpoint_dir", str(tmp_path / "ck"), "--test_dir", str(tmp_path / "out")])
    assert len(out) == 1 and os.path.exists(tmp_path / "out" / "aachen_000016.png") and os.path.exists(tmp_path / "out" / "real_aachen_000016.png")
    assert not [f for f in os.listdir(FIX) if f not in ("trainA", "trainA_seg", "trainA_seg_class", "testA", "testA_seg", "testA_seg_class")]
    # no trainA under that name: today's synthetic run
    hist = main(common[:-4] + ["--epoch", "1", "--dataset_dir", "unit", "--steps_per_epoch", "1", "--checkpoint_dir", str(tmp_path / "ck3"),
                               "--test_dir", str(tmp_path / "t3"), "--log_dir", str(tmp_path / "logs3")])
    assert len(hist) == 1 and os.path.exists(tmp_path / "t3" / "synthetic_000.png")
