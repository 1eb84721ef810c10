"""GPU tests of the layer walks that a network and its lockstep pair share (module._ResNetWalk / _UNetWalk) and of the unit
protocol they are written against: the order in which layers report completion -- what the data-parallel buckets hang
their all-reduces on -- and the limits of the lockstep units' backward."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import sggan_amd
    return sggan_amd.module


def _completion_order(net, x):
    done = []
    y, tape = net.forward(x)
    net.backward(tape, torch.ones_like(y), on_unit_done=done.append)
    torch.cuda.synchronize()
    return done


@pytest.mark.parametrize("arch,ckpt", [("resnet", False), ("resnet", True), ("unet", False)],
                         ids=["resnet", "resnet_checkpointed", "unet"])
def test_layers_complete_in_reverse_layer_order_single_and_pair(M, arch, ckpt):
    """``on_unit_done`` names every layer exactly once, in reverse ``conv_units()`` order, and a network and the lockstep
    pair of two such networks give the same list (model._bucketed_allreduce plans its buckets per network and launches them
    from the pair's one callback).  Generator(gf_dim=8, n_blocks=2) at 1x32x32 and GeneratorUNet(gf_dim=8) at 1x16x16, the
    pairs on the stacked 2-image batch; the ResNet also with activation checkpointing, whose recomputed blocks must not be
    reported (nor change the order)."""
    if arch == "resnet":
        nets = [M.Generator(gf_dim=8, n_blocks=2, dtype=torch.float32, seed=s) for s in (19, 21)]
        pair, hw = M.GeneratorPair(*nets), 32
    else:
        nets = [M.GeneratorUNet(gf_dim=8, dtype=torch.float32, seed=s) for s in (19, 21)]
        pair, hw = M.GeneratorUNetPair(*nets), 16
    for n in nets:
        n.checkpoint_blocks = ckpt
    gen = torch.Generator().manual_seed(5)
    xs = [n.to_internal(torch.rand(1, hw, hw, 3, generator=gen)) for n in nets]
    expect = [u.name for u in reversed(nets[0].conv_units())]
    assert len(set(expect)) == len(expect) == (10 if arch == "resnet" else 16)
    single = _completion_order(nets[0], xs[0])
    paired = _completion_order(pair, torch.cat(xs))
    assert single == expect
    assert paired == expect
    assert [u.name for u in reversed(pair.conv_units())] == expect
    assert not (nets[0].pending_wgrads() or nets[1].pending_wgrads())


def test_pair_unit_backward_keeps_the_unit_protocol_within_its_limits(M):
    """A lockstep unit runs the one backward of the units (_Unit.backward) but has no form for a caller's gradient buffer or for
    norm-backward sums made by the previous data gradient: both are refused (AssertionError, before anything is launched).
    With ``next_norm`` it returns (dx, None) -- its data-gradient epilogue never makes the next norm's sums -- and dx is the
    same bits as without.  One stride-1 SAME 3x3 conv + instance norm pair unit, 8 -> 8 channels, 2x16x16, f32 (the first
    encoder layer of two 8-channel-input U-Nets)."""
    ga, gb = (M.GeneratorUNet(gf_dim=8, in_c=8, dtype=torch.float32, seed=s) for s in (19, 21))
    pu = M.GeneratorUNetPair(ga, gb).enc[0]
    assert (pu.name, pu.ua.R, pu.ua.stride, pu.ua.padding, pu.ua.cin, pu.ua.cout, pu.skip_grad) == ("e1", 3, 1, "SAME", 8, 8, False)
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(2, 16, 16, 8, generator=gen).cuda()
    y, rec = pu.forward(x)
    dy = torch.randn(tuple(y.shape), generator=gen).cuda()
    with pytest.raises(AssertionError):
        pu.backward(rec, dy, gbuf=torch.zeros_like(ga.P.grad))
    with pytest.raises(AssertionError):
        pu.backward(rec, dy, dy_partial=torch.zeros(2, 1, 8, 2, device="cuda"))
    assert not ga.P.grad.any() and not gb.P.grad.any()            # the refused calls launched nothing
    dx = pu.backward(rec, dy)
    out = pu.backward(rec, dy, next_norm=(pu, rec))
    assert isinstance(out, tuple) and len(out) == 2 and out[1] is None
    assert dx.shape == x.shape and torch.equal(out[0], dx)
    assert ga.P.g("e1_w").abs().sum() > 0 and gb.P.g("e1_w").abs().sum() > 0
