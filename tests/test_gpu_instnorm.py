"""The instance-norm kernels of csrc/norm.hip -- plain, _partial, _mixed, _skip and _pair forms, the one-launch path for small
maps, sgg_instnorm_finalize -- against tests/instnorm_oracle.py (float64, written from include/sggan.h) at the shapes where
their chunking, tails and path switches change (the reasons stand next to each shape in instnorm_oracle.SHAPES).

Two input families.  EXACT: small integers with zero mean and var + eps a power of four, dy in eighths, power-of-two gamma,
leak 1/4 -- statistics, y, dx, dskip, dgamma and dbeta are compared for EQUALITY with the oracle rounded to the storage type
(rstd within one float32 ulp), so one dropped, doubled or misattributed pixel fails at any size; every even channel has a
group of pixels at a pre-activation of exactly 0.  RANDOM: normal data, judged PER ELEMENT against the bounds derived in
instnorm_oracle (stats per (n, c)); no maximum over a tensor's scale is taken and no element is left out.
tests/test_instnorm_oracle_cpu.py proves premise, kink margin and that the reference arithmetic itself meets the bounds
for every case here.  Outputs are pre-filled with NaN / sentinels."""
import ctypes

import numpy as np
import pytest
import torch

from tests import instnorm_oracle as I

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
F64 = np.float64
RATIOS = {}                                    # (output, dtype) -> largest err / bound seen on the random family


@pytest.fixture(scope="module")
def K():
    from sggan_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def A():
    from sggan_amd import _abi
    return _abi


def dev(a, name="f32"):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to("cuda").to(DT[name])


def host(t):
    return t.detach().float().cpu().numpy().astype(F64)


def nans(shape, name="f32"):
    return torch.full(tuple(shape), float("nan"), dtype=DT[name], device="cuda")


def same(got, exp, what):
    g, e = host(got), np.asarray(exp, F64)
    assert g.shape == e.shape, (what, g.shape, e.shape)
    assert not np.isnan(g).any(), f"{what}: {int(np.isnan(g).sum())} unwritten (NaN) elements"
    bad = g != e
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}: got {g[bad][0]!r}, expected {e[bad][0]!r}"


def inside(got, exp, bound, what, key, name):
    g, e, b = host(got), np.asarray(exp, F64), np.asarray(bound, F64)
    assert g.shape == e.shape == b.shape, (what, g.shape, e.shape, b.shape)
    assert np.isfinite(g).all(), f"{what}: {int((~np.isfinite(g)).sum())} non-finite (or unwritten) elements"
    err = np.abs(g - e)
    ratio = float((err / np.maximum(b, 1e-300)).max())
    RATIOS[(key, name)] = max(RATIOS.get((key, name), 0.0), ratio)
    print(f"{what}: max err / bound {ratio:.3f}")
    bad = err > b
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} outside the bound, worst err / bound {ratio:.3f} at "
                           f"{np.unravel_index(np.argmax(err / np.maximum(b, 1e-300)), e.shape)}")


class Run:
    """One case on the device: calls the entry points through sggan_amd.kernels and judges each output."""

    def __init__(self, K, spec, c_real=None, accumulate=False):
        self.K, self.spec, self.case = K, spec, I.build(spec)
        c = self.case
        self.name, self.exact = spec["name"], spec["family"] == "exact"
        self.x64 = c["x"]
        self.N, self.H, self.W, self.C = self.x64.shape
        self.HW = self.H * self.W
        self.act, self.leak, self.eps, self.pair = c["act"], c["leak"], c["eps"], c["pair"]
        self.x, self.gamma, self.beta = dev(c["x"], self.name), dev(c["gamma"]), dev(c["beta"])
        if self.pair:
            self.gamma2, self.beta2, self.ns = dev(c["gamma2"]), dev(c["beta2"]), self.pair[2]
        self.mean, self.rstd = I.stats(self.x64, self.eps)
        self.stats = dev(np.stack([self.mean, self.rstd], -1))       # the oracle's statistics rounded to float32: the backward's input
        self.c_real, self.accumulate = c_real or self.C, accumulate
        self.out = {}                                                # every output tensor, by call, for the determinism test

    def rel(self, one_launch):
        return I.sum_rel(self.name, I.chain_pixels(self.HW, one_launch))

    # ---- forward
    def check_forward(self, tag, y, stats, rel, residual=None, skip=None):
        c = self.case
        self.out[tag] = (y, stats)
        kw = dict(residual=None if residual is None else c["residual"], skip=None if skip is None else c["skip"], pair=self.pair)
        ye = I.forward(self.x64, c["gamma"], c["beta"], self.eps, self.act, self.leak, **kw)[0]
        what = f"{self.spec['id']} {tag}"
        assert tuple(stats.shape) == (self.N, self.C, 2)
        if self.exact:
            same(stats[..., 0], self.mean, what + " mean")
            sr = host(stats[..., 1])
            assert (np.abs(sr - self.rstd) <= I.ulp(self.rstd, "f32")).all(), what + " rstd"
            same(y, I.to_storage(ye, self.name), what + " y")
        else:
            bm, br = I.stats_bounds(self.x64, self.eps, rel)
            inside(stats[..., 0], self.mean, bm, what + " mean", "stats", self.name)
            inside(stats[..., 1], self.rstd, br, what + " rstd", "stats", self.name)
            by = I.forward_bounds(self.x64, c["gamma"], c["beta"], self.eps, self.act, self.leak, self.name, rel, **kw)[0]
            inside(y, ye, by, what + " y", "y", self.name)
        return ye

    def forward_all(self, partial=True, skip=True):
        K, c = self.K, self.case
        a = (self.eps, self.act, self.leak)
        res, sk = dev(c["residual"], self.name), dev(c["skip"], self.name)
        rows = dev(I.partial_rows(self.x64, I.chunks(self.HW))) if partial else None
        rel_rows = I.sum_rel("f32", self.HW)                         # float64 sums cast to float32 once per chunk, whatever the tensor's type
        if self.pair:
            p = (self.gamma, self.beta, self.gamma2, self.beta2, self.ns)
            self.check_forward("fwd_pair", *K.instnorm_fwd_pair(self.x, *p, None, *a), self.rel(True))
            self.check_forward("fwd_pair+res", *K.instnorm_fwd_pair(self.x, *p, res, *a), self.rel(True), residual=True)
            self.check_forward("fwd_partial_pair", *K.instnorm_fwd_partial_pair(self.x, rows, *p, res, *a), rel_rows, residual=True)
            self.check_forward("fwd_skip_pair", *K.instnorm_fwd_skip_pair(self.x, *p, sk, *a), self.rel(False), skip=True)
            self.check_forward("fwd_skip_partial_pair", *K.instnorm_fwd_skip_pair(self.x, *p, sk, *a, partial=rows), rel_rows, skip=True)
            return
        p = (self.gamma, self.beta)
        self.check_forward("fwd", *K.instnorm_fwd(self.x, *p, None, *a), self.rel(True))
        self.check_forward("fwd+res", *K.instnorm_fwd(self.x, *p, res, *a), self.rel(True), residual=True)
        if partial:
            self.check_forward("fwd_partial", *K.instnorm_fwd_partial(self.x, rows, *p, None, *a), rel_rows)
            self.check_forward("fwd_partial+res", *K.instnorm_fwd_partial(self.x, rows, *p, res, *a), rel_rows, residual=True)
        if skip:
            self.check_forward("fwd_skip", *K.instnorm_fwd_skip(self.x, *p, sk, *a), self.rel(False), skip=True)
            if partial:
                self.check_forward("fwd_skip_partial", *K.instnorm_fwd_skip(self.x, *p, sk, *a, partial=rows), rel_rows, skip=True)

    # ---- backward
    SENTINEL = (np.arange(64) % 7 - 3) * 0.5

    def grads(self):
        """Parameter-gradient buffers, C long: NaN, or the sentinel pattern when C_real < C or accumulating; the kernels get views
        of the first C_real entries (sggan_amd.kernels takes C_real from their length)."""
        keys = ("dgamma", "dbeta") + (("dgamma2", "dbeta2") if self.pair else ())
        if self.c_real == self.C and not self.accumulate:
            full = {k: nans((self.C,)) for k in keys}
        else:
            full = {k: dev((i + 1) * self.SENTINEL[:self.C]) for i, k in enumerate(keys)}
        return full, [full[k][:self.c_real] for k in keys]

    def check_backward(self, tag, dx, full, dy64, rel, dskip=None, skip=False, name=None):
        c, name = self.case, name or self.name
        self.out[tag] = (dx, dskip) + tuple(full.values())
        o = I.backward(dy64, self.x64, c["gamma"], c["beta"], self.mean, self.rstd, self.act, self.leak, c["skip"] if skip else None, self.pair)
        what = f"{self.spec['id']} {tag}"
        base = {k: (i + 1) * self.SENTINEL[:self.C] for i, k in enumerate(full)}
        if not self.exact:
            b = I.backward_bounds(dy64, self.x64, c["gamma"], c["beta"], self.mean, self.rstd, self.act, self.leak, name, rel,
                                  skip=c["skip"] if skip else None, pair=self.pair, store_g=skip, accumulate_onto=base if self.accumulate else None)
        for k, buf in full.items():
            exp = o[k] + (base[k] if self.accumulate else 0.0)
            if self.exact:
                same(buf[:self.c_real], exp.astype(np.float32).astype(F64)[:self.c_real], f"{what} {k}")
            else:
                inside(buf[:self.c_real], exp[:self.c_real], b[k][:self.c_real], f"{what} {k}", k.rstrip("2"), name)
            if self.c_real < self.C:                                 # past C_real the buffer keeps its contents, bit for bit
                keep = np.asarray(base[k][self.c_real:], np.float32)
                assert np.array_equal(buf[self.c_real:].cpu().numpy().view(np.uint32), keep.view(np.uint32)), f"{what} {k}: written past C_real"
        for k, t in (("dx", dx),) + ((("dskip", dskip),) if dskip is not None else ()):
            if self.exact:
                same(t, I.to_storage(o[k], name), f"{what} {k}")
            else:
                inside(t, o[k], b[k], f"{what} {k}", "dx", name)
        return o

    def backward_all(self, partial=True, skip=True, mixed=True):
        K, c = self.K, self.case
        acc, a = self.accumulate, (self.act, self.leak)
        dy, dys = dev(c["dy"], self.name), dev(c["dy_skip"], self.name)
        y_skip = I.to_storage(I.forward(self.x64, c["gamma"], c["beta"], self.eps, self.act, self.leak, skip=c["skip"], pair=self.pair)[0], self.name)
        if self.pair:
            p = (self.gamma, self.beta, self.gamma2, self.beta2, self.ns)
            full, v = self.grads()
            self.check_backward("bwd_pair", K.instnorm_bwd_pair(dy, self.x, *p, self.stats, *v, acc, *a), full, c["dy"], self.rel(True))
            full, v = self.grads()
            dx, dskip = K.instnorm_bwd_skip_pair(dys, dev(y_skip, self.name), self.x, *p, self.stats, *v, acc, *a)
            self.check_backward("bwd_skip_pair", dx, full, c["dy_skip"], self.rel(False), dskip, skip=True)
            return
        p = (self.gamma, self.beta)
        full, v = self.grads()
        self.check_backward("bwd", K.instnorm_bwd(dy, self.x, *p, self.stats, *v, acc, *a), full, c["dy"], self.rel(True))
        if partial:
            rows = dev(I.bwd_partial_rows(c["dy"], self.x64, c["gamma"], c["beta"], self.mean, self.rstd, self.act, self.leak, I.chunks(self.HW)))
            full, v = self.grads()
            self.check_backward("bwd_partial", K.instnorm_bwd_partial(dy, self.x, rows, *p, self.stats, *v, acc, *a), full, c["dy"],
                                I.sum_rel("f32", self.HW))
        if mixed and self.name == "bf16":                            # f32 gradient of a bf16 tensor
            dy32 = c.get("dy32", c["dy"])
            full, v = self.grads()
            self.check_backward("bwd_mixed", K.instnorm_bwd(dev(dy32), self.x, *p, self.stats, *v, acc, *a), full, dy32, self.rel(False))
        if skip:
            full, v = self.grads()
            dx, dskip = K.instnorm_bwd_skip(dys, dev(y_skip, self.name), self.x, *p, self.stats, *v, acc, *a)
            self.check_backward("bwd_skip", dx, full, c["dy_skip"], self.rel(False), dskip, skip=True)


def ids(specs):
    return [s["id"] for s in specs]


# ---------------------------------------------------------------------------- the shape grid
@pytest.mark.parametrize("spec", I.specs_of("shape"), ids=ids(I.specs_of("shape")))
def test_every_form_at_the_chunk_tail_and_path_edges(K, spec):
    """Forward plain (+ residual), _partial, _skip, _skip_partial; backward plain, _partial, _mixed (bf16), _skip -- stats, y, dx,
    dskip, dgamma, dbeta against the oracle; the activations are spread over the grid."""
    r = Run(K, spec)
    r.forward_all()
    r.backward_all()


def test_129_chunks_and_2049_blocks(K):
    """524289 pixels: the second trip of the finalize reduction (chunks >= 128) and 256-pixel apply blocks; exact family, f32."""
    (spec,) = I.specs_of("big")
    r = Run(K, spec)
    assert I.chunks(r.HW) == 129
    r.forward_all(partial=False, skip=False)
    r.backward_all(partial=False, skip=True, mixed=False)


# ---------------------------------------------------------------------------- the caller's chunk count
@pytest.mark.parametrize("spec", I.specs_of("chunks"), ids=ids(I.specs_of("chunks")))
def test_caller_supplied_chunk_counts(K, spec):
    """sgg_instnorm_finalize, _fwd_partial, _fwd_skip_partial and _bwd_partial on statistics rows with the caller's chunk count:
    one trip of the finalize reduction, its lane count +- 1, its four-deep unroll +- 1 (128 +- 1), and well past it."""
    r = Run(K, spec)
    c = r.case
    rel = I.sum_rel("f32", r.HW)
    for nchunks in I.CHUNK_COUNTS:
        r.spec = dict(spec, id=f"{spec['id']} chunks={nchunks}")
        rows = dev(I.partial_rows(r.x64, nchunks))
        st = K.instnorm_finalize(rows, r.HW, r.eps)
        if r.exact:
            same(st[..., 0], r.mean, "finalize mean")
            assert (np.abs(host(st[..., 1]) - r.rstd) <= I.ulp(r.rstd, "f32")).all()
        else:
            bm, br = I.stats_bounds(r.x64, r.eps, rel)
            inside(st[..., 0], r.mean, bm, f"finalize mean chunks={nchunks}", "stats", r.name)
            inside(st[..., 1], r.rstd, br, f"finalize rstd chunks={nchunks}", "stats", r.name)
        a = (r.eps, r.act, r.leak)
        r.check_forward("fwd_partial", *K.instnorm_fwd_partial(r.x, rows, r.gamma, r.beta, None, *a), rel)
        r.check_forward("fwd_skip_partial", *K.instnorm_fwd_skip(r.x, r.gamma, r.beta, dev(c["skip"], r.name), *a, partial=rows), rel, skip=True)
        brows = dev(I.bwd_partial_rows(c["dy"], r.x64, c["gamma"], c["beta"], r.mean, r.rstd, r.act, r.leak, nchunks))
        full, v = r.grads()
        dx = K.instnorm_bwd_partial(dev(c["dy"], r.name), r.x, brows, r.gamma, r.beta, r.stats, *v, False, r.act, r.leak)
        r.check_backward("bwd_partial", dx, full, c["dy"], rel)


# ---------------------------------------------------------------------------- two networks in lockstep
@pytest.mark.parametrize("spec", I.specs_of("pair"), ids=ids(I.specs_of("pair")))
def test_pair_forms_against_the_two_network_oracle(K, spec):
    """_fwd_pair, _fwd_partial_pair, _bwd_pair, _fwd_skip_pair, _fwd_skip_partial_pair, _bwd_skip_pair against the oracle's
    two-network statement (not against the single forms): visibly different parameter sets, all four parameter gradients."""
    r = Run(K, spec)
    assert np.abs(r.case["gamma"] - r.case["gamma2"]).min() > 0
    r.forward_all()
    r.backward_all()


# ---------------------------------------------------------------------------- accumulate, C_real
@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("spec", I.specs_of("sentinel"), ids=ids(I.specs_of("sentinel")))
def test_accumulate_and_c_real_leave_the_rest_alone(K, spec, accumulate):
    """dgamma / dbeta (both sets) pre-filled with a sentinel pattern, C = 40 and C_real = 34: the first 34 entries are overwritten
    or added to, entries 34..39 keep their bits -- on the one-launch and on the split path, every backward form."""
    r = Run(K, spec, c_real=I.C_REAL, accumulate=accumulate)
    assert r.C == 40
    r.backward_all()


# ---------------------------------------------------------------------------- the kink
@pytest.mark.parametrize("spec", I.specs_of("kink"), ids=ids(I.specs_of("kink")))
def test_slope_at_a_pre_activation_of_exactly_zero(K, spec):
    """Pixels planted at z == 0 (and pixels on either side of it) in every even channel: dx and dskip are exact for RELU (slope
    0 at the kink) and LRELU (slope leak) on the plain, mixed and skip backwards."""
    r = Run(K, spec)
    c = r.case
    for skip in (None, c["skip"]):
        pre = I.forward(r.x64, c["gamma"], c["beta"], r.eps, r.act, r.leak, skip=skip)[3]
        assert (pre == 0).sum() >= r.N * r.C // 2 and (pre > 0).any() and (pre < 0).any()
    assert c["pattern"] == "zeros"
    r.forward_all(partial=False)
    r.backward_all(partial=False)
    # the convention itself, spelled out on the planted pixels of the plain backward
    pre = I.forward(r.x64, c["gamma"], c["beta"], r.eps, r.act, r.leak)[3]
    o = I.backward(c["dy"], r.x64, c["gamma"], c["beta"], r.mean, r.rstd, r.act, r.leak)
    at = pre == 0
    assert np.array_equal(o["g"][at], c["dy"][at] * (0.0 if r.act == I.RELU else r.leak))
    same(r.out["bwd"][0], I.to_storage(o["dx"], r.name), "dx at and around the kink")


# ---------------------------------------------------------------------------- degenerate statistics
@pytest.mark.parametrize("spec", I.specs_of("degenerate"), ids=ids(I.specs_of("degenerate")))
def test_degenerate_channels(K, spec):
    """Channel 0 constant (var = 0), channel 1 a constant that float32 sums cannot hold exactly (var must clamp at 0: rstd finite
    and 1/sqrt(eps) within the bound), channel 2 mean 50 over std 0.5 (E[x^2] - mean^2 cancels: the bound widens and holds)."""
    r = Run(K, spec)
    c = r.case
    r.forward_all()
    r.backward_all()
    for tag, (y, stats) in [(t, v) for t, v in r.out.items() if t.startswith("fwd")]:
        assert torch.isfinite(y.float()).all() and torch.isfinite(stats).all(), tag
    for tag, outs in [(t, v) for t, v in r.out.items() if t.startswith("bwd")]:
        assert all(torch.isfinite(t.float()).all() for t in outs if t is not None), tag
    assert np.allclose(r.rstd[:, :2], 1 / np.sqrt(I.f32(r.eps)))
    # y of a constant channel is act(beta) (+ residual), within the bound (which carries a |x A| term: not bit-equal)
    ye = I.forward(r.x64, c["gamma"], c["beta"], r.eps, r.act, r.leak)[0]
    assert np.array_equal(ye[..., 0], np.broadcast_to(I.act_fwd(c["beta"][0], r.act, r.leak), ye[..., 0].shape))
    by = I.forward_bounds(r.x64, c["gamma"], c["beta"], r.eps, r.act, r.leak, r.name, r.rel(True))[0]
    inside(r.out["fwd"][0][..., :2], np.broadcast_to(I.act_fwd(c["beta"][:2], r.act, r.leak), ye[..., :2].shape), by[..., :2],
           "y of the constant channels", "y", r.name)


# ---------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("spec", [s for s in I.specs_of("shape") + I.specs_of("pair") if s["family"] == "random" and
                                  (s["N"], s["H"], s["W"], s["C"], s["pair"]) in ((2, 8, 8, 40, None), (2, 19, 27, 40, None), (2, 8, 8, 40, 1), (2, 19, 27, 40, 1))],
                         ids=lambda s: s["id"])
def test_every_entry_point_is_deterministic(K, spec):
    """Each entry point twice on the same inputs, on a one-launch and a split shape: all outputs bit-equal."""
    runs = []
    for _ in range(2):
        r = Run(K, spec)
        r.forward_all()
        r.backward_all()
        runs.append(r.out)
    assert runs[0].keys() == runs[1].keys() and len(runs[0]) >= 7
    for tag in runs[0]:
        for a, b in zip(runs[0][tag], runs[1][tag]):
            if a is not None:
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{spec['id']} {tag}: two runs differ"


# ---------------------------------------------------------------------------- return codes
SIG = {
    "fwd": "x gamma beta residual y stats N HW C eps act leak dtype ws ws_bytes stream",
    "fwd_partial": "x gamma beta residual y stats partial chunks N HW C eps act leak dtype stream",
    "bwd": "dy x gamma beta stats dx dgamma dbeta N HW C C_real accumulate act leak dtype ws ws_bytes stream",
    "bwd_mixed": "dy x gamma beta stats dx dgamma dbeta N HW C C_real accumulate act leak ws ws_bytes stream",
    "bwd_partial": "dy x gamma beta stats dx dgamma dbeta partial chunks N HW C C_real accumulate act leak dtype ws ws_bytes stream",
    "fwd_pair": "x gamma beta gamma2 beta2 nsplit residual y stats N HW C eps act leak dtype ws ws_bytes stream",
    "fwd_partial_pair": "x gamma beta gamma2 beta2 nsplit residual y stats partial chunks N HW C eps act leak dtype stream",
    "bwd_pair": "dy x gamma beta gamma2 beta2 nsplit stats dx dgamma dbeta dgamma2 dbeta2 N HW C C_real accumulate act leak dtype ws ws_bytes stream",
    "fwd_skip": "x gamma beta skip y stats N HW C eps act leak dtype ws ws_bytes stream",
    "fwd_skip_partial": "x gamma beta skip y stats partial chunks N HW C eps act leak dtype stream",
    "bwd_skip": "dy yin x gamma beta stats dx dskip dgamma dbeta N HW C C_real accumulate act leak dtype ws ws_bytes stream",
    "fwd_skip_pair": "x gamma beta gamma2 beta2 nsplit skip y stats N HW C eps act leak dtype ws ws_bytes stream",
    "fwd_skip_partial_pair": "x gamma beta gamma2 beta2 nsplit skip y stats partial chunks N HW C eps act leak dtype stream",
    "bwd_skip_pair": "dy yin x gamma beta gamma2 beta2 nsplit stats dx dskip dgamma dbeta dgamma2 dbeta2 N HW C C_real accumulate act leak dtype ws ws_bytes stream",
}
OUTPUTS = ("y", "stats", "dx", "dskip", "dgamma", "dbeta", "dgamma2", "dbeta2")


class Abi:
    """Valid arguments of every entry point at (3, 9, 9, 16) (mixed: bf16 x, f32 dy), outputs filled with a sentinel; call() swaps
    some in, returns the status and checks that a refused call wrote nothing."""
    N, H, W, C = 3, 9, 9, 16

    def __init__(self, K, A, name):
        self.K, self.A, self.name = K, A, name
        rng = np.random.default_rng(31)
        shp = (self.N, self.H, self.W, self.C)
        t = lambda nm=name: dev(rng.standard_normal(shp), nm)
        self.v = dict(x=t(), residual=t(), skip=t(), dy=t(), yin=t(), gamma=dev(np.ones(self.C)), beta=dev(np.zeros(self.C)),
                      gamma2=dev(np.ones(self.C)), beta2=dev(np.zeros(self.C)), stats=dev(np.ones((self.N, self.C, 2))),
                      partial=dev(np.ones((self.N, 2, self.C, 2))), chunks=2, nsplit=1, N=self.N, HW=self.H * self.W, C=self.C,
                      C_real=self.C, accumulate=0, eps=1e-3, act=I.RELU, leak=0.0, dtype=K.dt(DT[name]), stream=K._s())
        need = int(A.lib().sgg_instnorm_workspace(self.N, self.H * self.W, self.C))
        assert need >= self.N * self.C * 16
        self.v.update(ws=torch.zeros(need, dtype=torch.uint8, device="cuda"), ws_bytes=need)

    def call(self, fn, **over):
        v = dict(self.v)
        if fn == "bwd_mixed":
            v["dy"] = v["dy"].float()
        outs = {"y": torch.full_like(v["x"], 7.0), "dx": torch.full_like(v["x"], 7.0), "dskip": torch.full_like(v["x"], 7.0)}
        if fn.startswith("fwd"):
            outs["stats"] = torch.full_like(v["stats"], 7.0)
        for k in ("dgamma", "dbeta", "dgamma2", "dbeta2"):
            outs[k] = torch.full((self.C,), 7.0, device="cuda")
        v.update(outs)
        v.update(over)
        if v.get("alias"):                                             # dx aliasing another argument of the skip backward
            v["dx"] = v[v["alias"]]
        before = {k: t.clone() for k, t in v.items() if isinstance(t, torch.Tensor)}
        args = [self.K._p(v[k]) if isinstance(v[k], torch.Tensor) or v[k] is None else v[k] for k in SIG[fn].split()]
        rc = getattr(self.A.lib(), "sgg_instnorm_" + fn)(*args)
        torch.cuda.synchronize()
        if rc != self.A.OK:
            for k, t in before.items():
                assert torch.equal(t.view(torch.uint8), v[k].view(torch.uint8)), f"{fn}: a refused call wrote to {k}"
        return rc


@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_return_codes_and_nothing_written(K, A, name):
    abi = Abi(K, A, name)
    fns = [f for f in SIG if not (f == "bwd_mixed" and name == "f32")]
    for fn in fns:
        assert abi.call(fn) == A.OK, fn                                # the arguments are valid to begin with
        assert abi.call(fn, act=I.TANH) == A.EUNSUPPORTED, fn
        assert abi.call(fn, C=12) == A.EINVAL, fn                      # C % 8 != 0
        if "ws" in SIG[fn].split():
            need = abi.N * abi.C * 16 if fn == "bwd_partial" else abi.v["ws_bytes"]
            assert abi.call(fn, ws_bytes=need - 1) == A.EWORKSPACE, fn
            assert abi.call(fn, ws_bytes=need) == A.OK, fn
        if fn.endswith("_pair"):
            assert abi.call(fn, nsplit=0) == A.EINVAL and abi.call(fn, nsplit=abi.N) == A.EINVAL, fn
            assert abi.call(fn, gamma2=None) == A.EINVAL and abi.call(fn, beta2=None) == A.EINVAL, fn
            if fn.startswith("bwd"):
                assert abi.call(fn, dgamma2=None) == A.EINVAL and abi.call(fn, dbeta2=None) == A.EINVAL, fn
        if fn.startswith("bwd_skip"):
            for other in ("dskip", "dy", "x"):
                assert abi.call(fn, alias=other) == A.EINVAL, (fn, other)
    assert A.lib().sgg_instnorm_finalize(K._p(abi.v["partial"]), 2, K._p(abi.v["stats"]), abi.N, abi.H * abi.W, 12, 1e-3, K._s()) == A.EINVAL


def test_zz_largest_err_over_bound_ratios():
    """Not a check of its own: prints the largest err / bound per output and dtype seen by the tests above (DESIGN.md section 16
    quotes them), and insists that the random family was judged at all."""
    for key in sorted(RATIOS):
        print(f"largest err / bound  {key[0]:7s} {key[1]:5s} {RATIOS[key]:.3f}")
    if RATIOS:
        assert {k[0] for k in RATIOS} >= {"stats", "y", "dx", "dgamma", "dbeta"} and max(RATIOS.values()) <= 1.0
