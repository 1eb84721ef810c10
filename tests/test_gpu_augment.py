"""Augmented training copy on the GPU: sgg_warp_affine_u8 against the float64 oracle (tests/augment_oracle.py on top of
tests/resample_oracle.py), sgg_resample_f32 against data.apply_tables, the doubled batch of DirectoryBatches(augment=True)
end to end on the fixture, and short training runs from the command line.

Bounds.  Warp, values in [0, 1]: |err| <= 1e-5 -- coordinates are float64 and evaluated exactly as the host does, weights
are non-negative and sum to 1, and a pixel is a sum of fewer than 100 f32 terms.  resample_f32: 1e-5 for the same reason as
resample_u8.  End to end: 2e-5 in f32 (two f32 stages), 2^-9 + 2e-5 in bf16.  Every case is compared in full."""
import os

import numpy as np
import pytest
import torch

import sggan_amd as sg
from sggan_amd import data as D
from sggan_amd import kernels as K
from tests import augment_oracle as AO
from tests import resample_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "city_small")
DEV = "cuda:0"
F32_TOL, BF16_TOL = 1e-5, 2.0 ** -9 + 1e-5
E2E_F32_TOL, E2E_BF16_TOL = 2e-5, 2.0 ** -9 + 2e-5


def _up(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x if dtype is None else np.asarray(x, dtype=dtype))).to(DEV)


def _warp(src, index, sets):
    """src (M,S,W0,Cs) uint8, sample k = source index[k] under parameter set sets[k] -> (N,S,S,4) f32 on the host."""
    M, S, W0, Cs = src.shape
    mats = D.augment_matrices(AO.stack(sets), S)
    cols, = D._device_tables((D.band_table((W0, S)),), DEV)
    out = torch.full((len(sets), S, S, 4), float("nan"), dtype=torch.float32, device=DEV)
    K.warp_affine_u8(_up(src), _up(index, np.int32), _up(mats), cols, D.warp_window(mats), out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), mats


def _check_warp(src, index, sets, tag):
    got, mats = _warp(src, index, sets)
    S = src.shape[1]
    squared = [O.resize(O.as_float(s)[..., :3], (S, S)) for s in src]
    worst = worst_spec = 0.0
    filled = 0
    for k, (i, p) in enumerate(zip(index, sets)):
        want, inside = AO.warp(squared[i], p)
        err = np.abs(got[k, ..., :3] - want).max()
        worst, worst_spec = max(worst, err), max(worst_spec, np.abs(got[k, ..., :3] - D.apply_augment(squared[i], mats[k])).max())
        filled += int(not inside.all())
        zero = ~D.augment_inside(mats[k], S)             # the decision the kernel is built to repeat (same float64 arithmetic)
        assert np.array_equal(got[k][zero], np.zeros_like(got[k][zero]))                # zero fill is exact
    print(f"{tag}: {len(sets)} samples ({filled} with zero fill), max|err| vs sequential oracle {worst:.3e}, vs data.apply_augment {worst_spec:.3e}")
    assert not np.isnan(got).any() and not got[..., 3].any()                            # written in full, channel 3 zero
    assert worst <= F32_TOL
    return worst


def test_warp_on_the_fixture_images_and_labels():
    """The city_small crops (1024x512 RGB images, RGBA labels): all six orders at both ends of every parameter range, plus
    drawn parameters."""
    cache = D.DatasetCache(FIX, "trainA", device="cpu")
    drawn = D.draw_augment_params(np.random.RandomState(23), 6)
    sets = AO.extremes() + [AO.one(drawn, i) for i in range(6)]
    for role in ("image", "label"):
        (key, src), = [(k, v.numpy()) for k, v in cache.stacks.items() if k[0] == role]
        assert key[1:3] == (512, 1024) and key[3] == (3 if role == "image" else 4)
        _check_warp(src, [k % len(src) for k in range(len(sets))], sets, f"fixture {role} Cs={key[3]}")


def test_warp_on_the_gta_geometry():
    """A synthetic 1052x1914 source (non-integer 1.82 squaring scale, ragged tiles: 1052 = 16 * 65 + 12 = 64 * 16 + 28)."""
    rng = np.random.default_rng(9)
    src = rng.integers(0, 256, (1, 1052, 1914, 3), dtype=np.uint8)
    src[0, :5, :9] = 255; src[0, -5:, -9:] = 0
    sets = AO.extremes()[::2] + AO.extremes()[1:2]          # every order; low, high and mixed ends
    _check_warp(src, [0] * len(sets), sets, "synthetic 1052x1914")


def test_warp_status_and_identity():
    """A window that cannot fit is refused, not shrunk; identity parameters return the squared image itself."""
    rng = np.random.default_rng(2)
    src = rng.integers(0, 256, (1, 96, 200, 4), dtype=np.uint8)
    ident = [AO.one(D.identity_augment_params(1), 0)]
    got, _ = _warp(src, [0], ident)
    assert np.abs(got[0, ..., :3] - O.resize(O.as_float(src[0])[..., :3], (96, 96))).max() <= F32_TOL
    cols, = D._device_tables((D.band_table((200, 96)),), DEV)
    out = torch.zeros((1, 96, 96, 4), dtype=torch.float32, device=DEV)
    mats = _up(D.augment_matrices(AO.stack(ident), 96))
    with pytest.raises(sg._abi.SggError):
        K.warp_affine_u8(_up(src), _up([0], np.int32), mats, cols, (96, 96), out)        # 96 * 96 * 16 B > 64 KB
    torch.cuda.synchronize()
    assert not out.any()


def _resample_f32(src, flip, tables, H, W, dtype, C=3, into=None):
    rows, cols = D._device_tables(tables, DEV)
    out = torch.full((len(src), H, W, 8), float("nan"), dtype=dtype, device=DEV) if into is None else into
    K.resample_f32(_up(src), _up(flip, np.int32), rows, cols, out, C)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("S,dst_hw", [(256, (64, 128)), (263, (64, 128)), (256, (32, 32)), (1024, (256, 512))])
def test_resample_f32_against_apply_tables(S, dst_hw):
    H, W = dst_hw
    rng = np.random.default_rng(S + W)
    n = 2 if S >= 1024 else 3
    src = rng.random((n, S, S, 4), dtype=np.float32)
    src[..., 3] = 0
    src[0, :4, :4] = 1.0; src[0, -4:, -4:] = 0.0
    flip = [1, 0, 1][:n]
    tables = (D.band_table((S, H)), D.band_table((S, W)))
    want = np.stack([D.apply_tables(s[..., :3], D.band_table64((S, H)), D.band_table64((S, W))) for s in src])
    want = np.stack([w[:, ::-1] if f else w for w, f in zip(want, flip)])
    out32 = _resample_f32(src, flip, tables, H, W, torch.float32)
    out16 = _resample_f32(src, flip, tables, H, W, torch.bfloat16)
    e32 = np.abs(out32[..., :3].cpu().numpy().astype(np.float64) - want).max()
    e16 = np.abs(out16[..., :3].float().cpu().numpy().astype(np.float64) - want).max()
    print(f"S={S}->{dst_hw}: taps {tables[0][0].shape[1]}x{tables[1][0].shape[1]}  f32 max|err| {e32:.3e}  bf16 max|err| {e16:.3e}")
    assert e32 <= F32_TOL
    assert torch.equal(out16, out32.to(torch.bfloat16))                    # bf16 = RNE of the f32 result, bit for bit
    assert e16 <= BF16_TOL
    assert torch.count_nonzero(out32[..., 3:]) == 0 and torch.count_nonzero(out16[..., 3:]) == 0 and not torch.isnan(out32).any()


def test_resample_f32_flip_position_and_stride_are_bit_exact():
    rng = np.random.default_rng(5)
    base = rng.random((3, 263, 263, 4), dtype=np.float32)
    t = (D.band_table((263, 64)), D.band_table((263, 128)))
    for dtype in (torch.float32, torch.bfloat16):
        a = _resample_f32(base[[0, 1, 2, 1, 1]], [0, 0, 0, 1, 0], t, 64, 128, dtype, C=4)
        b = _resample_f32(base[[1, 1, 0, 2, 1, 0, 1]], [1, 0, 1, 1, 0, 0, 1], t, 64, 128, dtype, C=4)
        assert torch.equal(a[3], a[1].flip(1))                             # flipped = unflipped reversed along W
        assert torch.equal(a[4], a[1]) and torch.equal(b[1], a[1]) and torch.equal(b[4], a[1]) and torch.equal(b[5], a[0])
        assert torch.equal(b[0], a[3]) and torch.equal(b[6], a[3]) and torch.equal(b[2], a[0].flip(1)) and torch.equal(b[3], a[2].flip(1))
        assert torch.count_nonzero(a[..., 3]) > 0 and torch.count_nonzero(a[..., 4:]) == 0      # C = 4 carries the fourth channel
        # the odd rows of a doubled batch: a strided destination gets the same bits and leaves the even rows alone
        buf = torch.full((6, 64, 128, 8), 7.0, dtype=dtype, device=DEV)
        _resample_f32(base, [0, 1, 0], t, 64, 128, dtype, C=4, into=buf[1::2])
        dense = _resample_f32(base, [0, 1, 0], t, 64, 128, dtype, C=4)
        assert torch.equal(buf[1::2], dense) and torch.equal(buf[0::2], torch.full_like(buf[0::2], 7.0))
        wide = _resample_f32(base[1:2], [0], (D.band_table((263, 64)), D.band_table((263, 263))), 64, 263, dtype)   # a ragged second tile
        ref = D.apply_tables(base[1, ..., :3], D.band_table64((263, 64)), D.band_table64((263, 263)))
        assert np.abs(wide[0, ..., :3].float().cpu().numpy() - ref).max() <= (F32_TOL if dtype == torch.float32 else BF16_TOL)


def _small_args(**kw):
    a = dict(ngf=8, ndf=8, n_blocks=2, batch_size=2, image_height=128, image_width=256, device=DEV, epoch=2, train_size=10 ** 8,
             checkpoint_dir=None, continue_train=False)
    a.update(kw)
    return sg.default_args(**a)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_doubled_batch_on_the_fixture(dtype):
    """Even rows: bit-identical to an augment=False loader on the same rng seed.  Odd rows: the float64 chain square -> warp
    -> resize -> flip on the PIL-decoded files.  Odd masks: the file's own mask with the copy's flip, exactly."""
    from PIL import Image
    from sggan_amd.segment_class import one_hot_mask
    args = _small_args(dtype=dtype, batch_size=2)
    model = sg.sggan(args)
    cache = D.DatasetCache(FIX, "trainA", device=DEV)
    plain = D.DirectoryBatches(model, args, cache, rng=np.random.RandomState(3))
    aug = D.DirectoryBatches(model, args, cache, rng=np.random.RandomState(3), augment=True, aug_rng=np.random.RandomState(29))
    shadow = D.DirectoryBatches.__new__(D.DirectoryBatches)          # the same draws again, on the host only
    shadow.args, shadow.domains, shadow.augment = args, aug.domains, True
    shadow.rng, shadow.aug_rng = np.random.RandomState(3), np.random.RandomState(29)
    H, W = args.image_height, args.image_width
    mh, mw = D.mask_grid(model, H, W)
    tol = E2E_F32_TOL if dtype == "f32" else E2E_BF16_TOL
    worst, flips_seen = 0.0, set()
    for ep in range(3):
        (order,), flips, n = shadow.epoch_plan()
        params, = shadow.augment_plan([order])
        it_p, it_a = plain(ep), aug(ep)
        assert len(it_p) == len(it_a) == n == 1
        for step, (bp, ba) in enumerate(zip(it_p, it_a)):
            for name in ("real_A", "seg_A", "mask_A"):
                assert ba[name].shape[0] == 4 and bp[name].shape[0] == 2 and ba[name].dtype == bp[name].dtype
                assert torch.equal(ba[name][0::2], bp[name])
            for i in range(2):
                k = step * 2 + i
                path = cache.files[order[k]]
                p, lf = AO.one(params, k), bool(params["loader_flip"][k])
                flips_seen.add(lf)
                for name, sub in (("real_A", ""), ("seg_A", "_seg")):
                    u8 = np.asarray(Image.open(D.sibling(path, "trainA", sub) if sub else path))
                    S = u8.shape[0]
                    warped, _ = AO.warp(O.resize(O.as_float(u8)[..., :3], (S, S)), p)
                    ref = O.resize(warped, (H, W))
                    ref = ref[:, ::-1] if lf else ref
                    got = ba[name][2 * i + 1]
                    err = np.abs(got[..., :3].float().cpu().numpy() - ref).max()
                    worst = max(worst, err)
                    print(f"{dtype} ep {ep} {os.path.basename(path)} {name} perm={p['perm']} loader_flip={lf}: max|err| {err:.3e}")
                    assert err <= tol and torch.count_nonzero(got[..., 3:]) == 0
                cls = np.asarray(Image.open(D.sibling(path, "trainA", "_seg_class")))
                m = one_hot_mask(cls, mh, mw, args.segment_class)[0]
                assert torch.equal(ba["mask_A"][2 * i + 1], m.flip(1) if lf else m)
    print(f"{dtype}: worst end-to-end max|err| {worst:.3e} (bound {tol:.3e})")
    assert flips_seen == {True, False}


def _main_args(tmp_path, tag, *extra):
    return ["--img_height", "128", "--img_width", "256", "--ngf", "8", "--ndf", "8", "--epoch", "1", "--dataset_dir", FIX,
            "--batch_size", "2", "--log_dir", str(tmp_path / ("logs" + tag)), "--checkpoint_dir", str(tmp_path / ("ck" + tag)),
            "--test_dir", str(tmp_path / ("test" + tag)), *extra]


def test_command_line_trains_on_the_doubled_batch(tmp_path, monkeypatch):
    """--augment in reference mode with the ResNet, eager and --graph: the step runs on 2 x batch_size images."""
    from sggan_amd.main import main
    from sggan_amd.model import sggan
    seen = []
    body = sggan._step_body
    monkeypatch.setattr(sggan, "_step_body", lambda self: (seen.append(tuple(self.real_A.shape)), body(self))[1])
    for tag, extra in (("e", []), ("g", ["--graph"])):
        del seen[:]
        hist = main(_main_args(tmp_path, tag, "--augment", *extra))
        assert len(hist) == 1 and np.isfinite(hist[0]["Generator Loss"]) and np.isfinite(hist[0]["Discriminator Loss"])
        assert seen and all(s == (4, 128, 256, 8) for s in seen), seen
    del seen[:]
    main(_main_args(tmp_path, "p"))
    assert seen and all(s[0] == 2 for s in seen)                       # without the flag: batch_size images, as before


@pytest.mark.parametrize("cycle", [False, True])
def test_graph_replay_reads_the_doubled_buffers_in_place(cycle):
    """Two epochs with --graph semantics: the step is recorded once, its static inputs ARE the loader's 2N buffers (same
    objects, same addresses before and after), and it ends bit-equal to the eager run.  Cycle mode fills all six buffers."""
    def train(graph):
        args = _small_args(dtype="bf16", batch_size=1, graph=graph, cycle=cycle)
        model = sg.sggan(args)
        records = []
        rec = model._record
        model._record = lambda: (records.append(1), rec())[1]
        cache = D.DatasetCache(FIX, "trainA", device=DEV)
        batches = D.DirectoryBatches(model, args, cache, cache if cycle else None, rng=np.random.RandomState(3), augment=True)
        ptrs = {k: v.data_ptr() for k, v in batches.batch.items()}
        hist = model.train(args, batches, log=lambda s: None)
        torch.cuda.synchronize()
        assert ptrs == {k: v.data_ptr() for k, v in batches.batch.items()}
        return model, hist, len(records), batches
    eager, h0, n0, _ = train(False)
    graph, h1, n1, batches = train(True)
    assert n0 == 0 and n1 == 1
    assert sorted(batches.batch) == sorted(["real_A", "seg_A", "mask_A"] + (["real_B", "seg_B", "mask_B"] if cycle else []))
    for k, v in batches.batch.items():
        assert v.shape[0] == 2 and graph._static_in[k] is v and getattr(graph, k) is v
        assert all(torch.count_nonzero(v[r].float()) > 0 for r in range(2)), k       # both rows of every buffer were filled
    assert len(h1) == 2 and all(np.isfinite(h["Generator Loss"]) and np.isfinite(h["Discriminator Loss"]) for h in h0 + h1)
    for a, b in zip(eager.networks(), graph.networks()):
        assert torch.isfinite(b.P.flat).all() and torch.equal(a.P.flat, b.P.flat)
    assert [h["Generator Loss"] for h in h0] == [h["Generator Loss"] for h in h1]
