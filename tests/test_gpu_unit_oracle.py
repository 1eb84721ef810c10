"""Every layer unit of module.py against the float64 unit of tests/unit_oracle.py, at the images where the units' launch choices
flip (the table of unit_oracle.ROWS; tests/test_unit_oracle_cpu.py asserts that table through the query functions).

One test per row: the network alone (not the model), parameters and inputs from the closed-form hash of test_gpu_adam_bits.py
-- every bias, gamma and beta away from its initial 0 / 1, so a bias or an affine pair handed to the wrong image shows --, one
forward and one backward of the real walk under the recorder of tests/unit_spy.py, then every recorded call against the
reference, teacher-forced on the tensors the device stored.  A failure names the row, the unit, the network of a pair, the
stage, the worst element and its bound.  The symbols the run called are recorded too: every row that claims a branch asserts
that the launch it names was made (or was not).  The worst error-to-bound ratio per stage is printed (run with -s)."""
import json
import math

import numpy as np
import pytest
import torch

from tests import unit_oracle as UO
from tests import unit_spy
from tests.test_gpu_adam_bits import hashed_f32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    return sggan_amd


class Names:
    """Stands where ``_abi._lib`` stands and keeps the name of every symbol that is called."""

    def __init__(self, real):
        self._real, self.names = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            self.names.append(name)
            return fn(*args)
        self.__dict__[name] = call
        return call


def hashed_params(net, stream):
    """Glorot-sized kernels, bias in 0.1 * [-1, 1), gamma in 1 + 0.25 * [-1, 1), beta in 0.25 * [-1, 1), all from hashed_f32."""
    out = {}
    for k, (name, shape) in enumerate(net.P.specs):
        shape = tuple(int(s) for s in shape)
        h = hashed_f32(stream + k, int(np.prod(shape))).reshape(shape)
        if name.endswith("_w"):
            rf = shape[0] * shape[1]
            out[name] = h * np.float32(math.sqrt(6.0 / (rf * (shape[2] + shape[3]))))
        elif name.endswith("_g"):
            out[name] = np.float32(1) + np.float32(0.25) * h
        else:
            out[name] = np.float32(0.1 if name.endswith("_b") else 0.25) * h
    return out


def build(sg, row):
    M = sg.module
    dt = {"bf16": torch.bfloat16, "f32": torch.float32}[row["dtype"]]
    nets = []
    for i in range(2 if row["pair"] else 1):
        if row["net"] == "resnet":
            net = M.Generator(gf_dim=row["width"], n_blocks=row["n_blocks"], dtype=dt, device="cuda", seed=None)
        elif row["net"] == "unet":
            net = M.GeneratorUNet(gf_dim=row["width"], dtype=dt, device="cuda", seed=None, dropout=row["dropout"])
            net.seed = 1234 + 17 * i
        else:
            net = M.Discriminator(df_dim=row["width"], dtype=dt, device="cuda", seed=None)
        net.P.load(hashed_params(net, 1000 * (i + 1)))
        for k, v in row["switches"].items():
            assert hasattr(net, k), k
            setattr(net, k, v)
        net.P.zero_grad()
        nets.append(net)
    if not row["pair"]:
        return nets, nets[0]
    pair = {"resnet": M.GeneratorPair, "unet": M.GeneratorUNetPair, "disc": M.DiscriminatorPair}[row["net"]]
    return nets, pair(*nets)


def apply_once(sg, row, nets, walk, image, stream):
    """One forward and one backward of the walk on hashed inputs."""
    K = sg.kernels
    H, W = image
    n = row["batch"] * len(nets)
    x = torch.from_numpy(hashed_f32(stream, n * H * W * 3).reshape(n, H, W, 3)).cuda()
    xi = nets[0].to_internal(x)
    if row["net"] == "disc":
        mh, mw = nets[0].out_hw(H, W)
        C = nets[0].segment_class
        idx = np.minimum(((hashed_f32(stream + 1, n * mh * mw) + np.float32(1)) * np.float32(0.5 * C)).astype(np.int64), C - 1)
        mask = np.zeros((n * mh * mw, C), np.float32)
        mask[np.arange(idx.size), idx] = 1.0
        out, tape = walk.forward(xi, torch.from_numpy(mask.reshape(n, mh, mw, C)).cuda())
        dy = torch.from_numpy(hashed_f32(stream + 2, out.numel()).reshape(tuple(out.shape))).cuda()
        return walk.backward(tape, dy, want_dx=True)
    if row["net"] == "unet" and row["dropout"]:
        out, tape = walk.forward(xi, dropout=0, sample_offset=0)
    else:
        out, tape = walk.forward(xi)
    dy = K.pad_channels(torch.from_numpy(hashed_f32(stream + 2, n * H * W * 3).reshape(n, H, W, 3)).cuda(), 8, nets[0].dtype)
    return walk.backward(tape, dy, want_dx=True)


@pytest.mark.parametrize("row", UO.ROWS, ids=[r["id"] for r in UO.ROWS])
def test_every_unit_against_float64(sg, row):
    A = sg._abi
    nets, walk = build(sg, row)
    want = UO.topology(row["net"], row["width"], row.get("n_blocks", 2))
    assert [UO.layer_of(u) for u in walk.conv_units()] == want
    torch.cuda.synchronize()
    real = A.lib()
    proxy = Names(real)
    A._lib = proxy
    try:
        with unit_spy.Spy(walk, A.route_name) as spy:
            for k in range(row.get("applications", 1)):
                apply_once(sg, row, nets, walk, row.get("second_image", row["image"]) if k else row["image"], 7 + 10 * k)
            for net in nets:
                net.flush_wgrads()
        torch.cuda.synchronize()
    finally:
        A._lib = real
    called = set(proxy.names)
    must, must_not = row["launches"]
    assert set(must) <= called and not (set(must_not) & called), (row["id"], sorted(set(must) - called), sorted(set(must_not) & called))
    report = {}
    results = unit_spy.check(spy, row["dtype"], report, row.get("only_net"))
    print(f"\nunit-oracle {row['id']}: {len(spy.calls)} calls; worst ratio per stage " + json.dumps({k: float(f'{v:.4g}') for k, v in sorted(report.items())}))
    bad = unit_spy.failures(results)
    assert not bad, f"{row['id']}: {len(bad)} stage(s) out of bounds\n  " + "\n  ".join(bad[:12])
    strays = [u.name for kind, u, c in spy.calls if kind == "backward" and not c["own_record"]]
    assert not strays, f"{row['id']}: backward of {strays} was handed a record its own forward did not return"
    # a unit is handed norm-backward sums exactly when the data gradient in front of it returned some, and it is the unit they were made for
    back = [(u.name, c) for kind, u, c in spy.calls if kind == "backward"]
    for (_, prev), (name, c) in zip([(None, None)] + back[:-1], back):
        made = prev is not None and prev["partial"] is not None
        assert c["had_dy_partial"] == made and (not made or prev["next"][3] == name), (row["id"], name)
    if row["switches"].get("fuse_in_bwd") and row["image"] in UO.FUSED_R:
        assert any(c["had_dy_partial"] for _, c in back)
    if row.get("live_backward"):
        assert all(bool(net.P.g("h0_w").abs().max() > 0) for net in nets), "the backward in front of h33 is identically zero"
    units = len(want)
    blocks = row.get("n_blocks", 2) if row["net"] == "resnet" else 0
    rerun = 2 * blocks if row["switches"].get("checkpoint_blocks") else 0            # (checkpointing re-runs the blocks' forwards)
    apps = row.get("applications", 1)
    assert sum(k == "forward" for k, _, _ in spy.calls) == apps * (units + rerun) and sum(k == "backward" for k, _, _ in spy.calls) == apps * units
