"""Data-parallel train step on the GPU box (one MI355X): the real ``sggan.train_step`` through
``enable_data_parallel()``.

* world size 1 over RCCL ("nccl"): async all-reduce + wait() + grad_scale through the real step, eager and as HIP-graph
  segments with the collectives between them -- must be bit-identical to the model without data parallelism.
* world size 2 (two processes sharing the one GPU, started by tests/dp_harness.py; gloo moves the CUDA buckets): each rank steps
  on its half of the batch; the averaged-gradient step must equal the single-process step on the concatenated batch,
  and the two replicas must stay bit-identical.
"""
import os
import socket
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _inputs(N, seed):
    g = torch.Generator().manual_seed(seed)
    real = torch.rand((N, 256, 256, 3), generator=g)
    seg = torch.rand((N, 256, 256, 3), generator=g)
    mask = torch.nn.functional.one_hot(torch.randint(0, 34, (N, 5, 5), generator=g), 34).float()
    return real, seg, mask


def _set(m, a, b, sl=slice(None)):
    m.real_A, m.seg_A, m.mask_A = (t[sl] for t in a)
    if m.cycle:
        m.real_B, m.seg_B, m.mask_B = (t[sl] for t in b)


@pytest.mark.parametrize("cycle", [False, True], ids=["reference", "cycle"])
def test_dp_world1_rccl_is_bit_identical_to_plain_step(cycle):
    import torch.distributed as dist
    import sggan_amd as sg
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        a, b = _inputs(2, 5), _inputs(2, 6)
        states = []
        for dp, graph in ((False, False), (True, False), (True, True)):
            m = sg.sggan(sg.default_args(ngf=16, ndf=16, n_blocks=2, dtype="f32", cycle=cycle, graph=graph))
            if dp:
                m.enable_data_parallel()
            _set(m, a, b)
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                for _ in range(2):
                    m.train_step()
            assert not [w for w in caught if "Graph is empty" in str(w.message)], "an empty HIP-graph segment was recorded"
            if dp and graph:
                # the collectives sit BETWEEN graph segments.  Host actions: one launch per discriminator bucket, one per
                # generator layer-group bucket (both generators of the paired cycle step share it), one wait per network;
                # actions with no launch between them share a cut, so graphs = cuts + 1 and the program starts and ends
                # with a graph
                kinds = [k for k, _ in m._program.items]
                plan = m.generator.bucket_plan(m.g_buckets)
                assert len(plan) >= 3 and plan[0][1] == 0 and plan[-1][2] == m.generator.P.numel
                assert all(a_[2] == b_[1] for a_, b_ in zip(plan, plan[1:]))
                n_d = len(m.networks()) // 2
                assert kinds.count("host") == n_d + len(plan) + len(m.networks())
                runs = sum(1 for i, k in enumerate(kinds) if k == "host" and (i == 0 or kinds[i - 1] != "host"))
                assert kinds[0] == "graph" and kinds[-1] == "graph" and kinds.count("graph") == runs + 1
                assert "graphgraph" not in "".join(kinds)
                if cycle:                                 # D_A's and D_B's launches are adjacent: they share one cut
                    assert runs < kinds.count("host")
            states.append([t.clone() for n in m.networks() for t in (n.P.flat, n.P.grad, n.P.m, n.P.v)] + [m._loss.clone()])
        for other in states[1:]:
            for x, y in zip(states[0], other):
                assert torch.equal(x, y)
    finally:
        dist.destroy_process_group()


def _worker(rank, world, graph):
    """One rank of the world-2 test (tests/dp_harness.py starts it in a fresh process, the process group initialised)."""
    import sggan_amd as sg
    m = sg.sggan(sg.default_args(ngf=16, ndf=16, n_blocks=2, dtype="f32", cycle=True, seed=19 + 7 * rank, graph=graph))
    m.enable_data_parallel()                      # broadcasts rank 0's state: replicas start identical
    a, b = _inputs(4, 5), _inputs(4, 6)
    _set(m, a, b, slice(2 * rank, 2 * rank + 2))
    m.train_step()
    gl, dl = m.losses()
    grads = [(n.P.grad / world).cpu().numpy() for n in m.networks()]       # buckets hold the SUM over ranks
    m.train_step()                                                          # a second step: replicas must not drift apart
    flat = torch.cat([n.P.flat for n in m.networks()]).cpu()
    return {1: flat.numpy(), 2: grads, 3: gl, 4: dl}


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_dp_world2_train_step_equals_concatenated_batch(graph):
    import sggan_amd as sg
    from tests import dp_harness
    res = dict(enumerate(dp_harness.launch(_worker, [graph, graph])))
    print("transport:", res[0]["transport"])
    assert np.array_equal(res[0][1], res[1][1])                     # replicas bit-identical after two steps
    assert all(np.array_equal(a, b) for a, b in zip(res[0][2], res[1][2]))
    # single process, concatenated batch, same initial parameters (rank 0's seed): the averaged gradients of step 1
    m = sg.sggan(sg.default_args(ngf=16, ndf=16, n_blocks=2, dtype="f32", cycle=True, seed=19))
    _set(m, _inputs(4, 5), _inputs(4, 6))
    m.train_step()
    errs = []
    for name, net, g_dp in zip(("G_AB", "D_A", "G_BA", "D_B"), m.networks(), res[0][2]):
        g = net.P.grad.cpu().numpy()
        # relative L2.  What this bound holds is the comparison of two f32 runs with each other, not the kernels' error: against
        # float64 with every ReLU / LeakyReLU kink and every sign() of the L1 / gradient-sensitive terms taken the device's way,
        # the exchanged buffers of a world-2 step are within 1.5e-5 of the sum of the ranks' oracle gradients in every tensor
        # (tests/test_gpu_dp_options.py, bound 2e-4).  Here nothing aligns those decisions: the pixel-split / split-K partitions
        # (hence the f32 summation order) depend on the per-rank batch size, the two runs' fakes differ in their last bits, and
        # every sign() argument or pre-activation that lands on the other side of zero moves its element's gradient by a whole
        # step (2 lambda / count for a sign); D's tail runs InstanceNorm over 5x5 maps with rstd up to 31.6.  Measured on an
        # MI355X: 2.4e-3 (G_AB), 7e-4 (G_BA), 8e-4 (D_B), 1.3e-4 (D_A) -- the count of flipped decisions is a property of this
        # seed's images, not derivable, so the bound stays at about twice the largest; a wrong mask, offset or clip factor is
        # tests/test_gpu_dp_options.py's to find, at its bounds
        errs.append((name, float(np.linalg.norm(g_dp - g) / np.linalg.norm(g))))
    print("DP(2 ranks) vs concatenated batch, relative L2 error of the averaged gradients:", errs)
    assert all(e < 5e-3 for _, e in errs), errs
    # each rank's loss is the mean over ITS samples; their average is the concatenated-batch loss
    gl, dl = m.losses()
    assert abs((res[0][3] + res[1][3]) / 2 - gl) < 1e-3 * abs(gl) and abs((res[0][4] + res[1][4]) / 2 - dl) < 1e-3 * abs(dl)
