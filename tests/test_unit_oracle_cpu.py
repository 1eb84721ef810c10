"""tests/unit_oracle.py without a GPU: (1) the case table says what the library's query functions say, so a later change of a
selection predicate fails here instead of quietly moving a case to the other side of its flip; (2) the float64 unit agrees with
finite differences on a tiny unit of each kind; (3) the checks are sensitive: a correct float64 result rounded to the storage
type passes, and the same result with one planted error -- a border row replaced by its neighbour, a tap dropped, a statistics
chunk counted twice, the addend left out, the two networks' weights swapped in the second half of a stacked batch -- fails."""
import numpy as np
import pytest

from tests import instnorm_oracle as I
from tests import unit_oracle as UO

F64 = np.float64


@pytest.fixture(scope="module")
def sg():
    import sggan_amd
    return sggan_amd


# ---------------------------------------------------------------------------- (1) the table
@pytest.mark.parametrize("row", UO.ROWS, ids=[r["id"] for r in UO.ROWS])
def test_table_matches_the_query_functions(sg, row):
    K, A = sg.kernels, sg._abi
    geoms, stacked = UO.plan(K, row), UO.plan(K, row, N=2 * row["batch"])
    assert row["expect"], row["id"]
    for key, fields in row["expect"].items():
        for name in UO.expected_layers(row, key):
            # ("pair" is asked of the stacked batch of both networks: that is the geometry the lockstep unit asks)
            got = dict(UO.describe(A, geoms[name]), pair=UO.describe(A, stacked[name])["pair"])
            assert {f: got[f] for f in fields} == fields, (row["id"], name, got)
    if row["pair"]:
        # the other flags must not differ between one network's share and the stack: the unit reads them from either
        flags = lambda g: {k: v for k, v in UO.describe(A, g).items() if k in ("stats", "bwd_stats", "wgrad_pair", "mixed", "normload")}
        for name, g in geoms.items():
            assert flags(stacked[name]) == flags(g), (row["id"], name)
    if row.get("second_image"):
        # the fallback of the deferred pair: the second application's residual layers are pairable too, at another shape
        other = UO.plan(K, dict(row, image=row["second_image"]))
        for name in UO.expected_layers(row, "r"):
            assert other[name].wgrad_pair and geoms[name].wgrad_pair and other[name].x_shape != geoms[name].x_shape


def test_s2halo_height_is_the_smallest(sg):
    K, A = sg.kernels, sg._abi
    base = dict(net="resnet", width=64, dtype="bf16", batch=2)
    takes = lambda H: (lambda g: A.route_name(g["d1"].route_fwd) == "S2HALO" and A.route_name(g["c3"].route_dgrad) == "S2HALO")(
        UO.plan(K, dict(base, image=(H, 512))))
    assert takes(128) and takes(UO.S2HALO_MIN_HEIGHT)
    assert not any(takes(H) for H in range(16, UO.S2HALO_MIN_HEIGHT, 4))


def test_discriminator_maps_with_live_pads(sg):
    row = UO.ROW_BY_ID["disc64-bf16-116x132-single"]
    geoms = UO.plan(sg.kernels, row)
    assert tuple(tuple(g.y_shape[1:3]) for g in geoms.values()) == UO.DISC_MAPS_116x132
    # asymmetric SAME pads (an odd map under stride 2) and a VALID row that no window reaches
    assert geoms["h2"].x_shape[1:3] == (29, 33) and geoms["h32"].x_shape[1:3] == (7, 8)


def test_unet_second_size_leaves_halo3(sg):
    A = sg._abi
    assert {"unet16-bf16-128x128-pair-net_a", "unet16-bf16-128x128-pair-dropout-net_b"} <= set(UO.ROW_BY_ID)
    for image, halo in (((128, 128), True), ((32, 32), False)):
        geoms = UO.plan(sg.kernels, UO.ROW_BY_ID[f"unet16-bf16-{image[0]}x{image[1]}-single"])
        for i in range(4, 9):
            assert (A.route_name(geoms[f"e{i}"].route_fwd) == "HALO3") == halo and (A.route_name(geoms[f"e{i}"].route_dgrad) == "HALO3") == halo


def test_topology_restates_the_parameter_specs(sg):
    M = sg.module
    for net, width, specs in (("resnet", 64, M.generator_param_specs(64, n_blocks=2)), ("disc", 64, M.discriminator_param_specs(64)),
                              ("unet", 16, M.unet_param_specs(16))):
        shapes = dict(specs)
        for L in UO.topology(net, width):
            want = (L.R, L.R, L.cin, L.cout) if L.kind == "conv" else (L.R, L.R, L.cout, L.cin)
            assert tuple(shapes[L.name + "_w"]) == want and ((L.name + "_g") in shapes) == L.norm, L


# ---------------------------------------------------------------------------- a host stand-in for the device
def params(L, seed, scale=0.3):
    rng = np.random.default_rng([77, seed])
    shape = (L.R, L.R, L.cin, L.cout) if L.kind == "conv" else (L.R, L.R, L.cout, L.cin)
    P = {L.name + "_w": rng.standard_normal(shape) * scale, L.name + "_b": rng.standard_normal(L.cout) * 0.1}
    if L.norm:
        P[L.name + "_g"] = 1 + 0.2 * rng.standard_normal(L.cout)
        P[L.name + "_beta"] = 0.2 * rng.standard_normal(L.cout)
    return P


def padded(a, name):
    """(N,H,W,C) values -> Rec with the channels padded with zeros."""
    a = np.asarray(a, F64)
    out = np.zeros(a.shape[:-1] + (UO.cpad(a.shape[-1]),), F64)
    out[..., :a.shape[-1]] = a
    return UO.Rec(out, name)


def host_forward(L, P, x, name, residual=None, exact=False, chunk_twice=None, eps=UO.EPS):
    """What a correct device stores for one forward call: float64 results, each rounded once to its storage type (exact: not
    rounded at all, for the finite differences).  chunk_twice: (chunks, k) -- statistics from rows of which row k counts twice."""
    q = (lambda a: np.asarray(a, F64)) if exact else (lambda a: I.to_storage(a, name))
    q32 = (lambda a: np.asarray(a, F64)) if exact else (lambda a: np.asarray(a, np.float32).astype(F64))
    conv = UO.conv_forward(L, x, P[L.name + "_w"], P[L.name + "_b"])[0]
    call = dict(x=padded(x, name), residual=None if residual is None else padded(residual, name), record_only=False, drop=None, stats_chunks=0,
                stats=None, y=None)
    if not L.norm:
        call["xc"] = padded(q(UO.act_forward(conv, 0.0, L)[0]), name)
        return call
    xc = q(conv)
    call["xc"] = padded(xc, name)
    if chunk_twice is None:
        mean, rstd = I.stats(xc, eps)
    else:
        rows = I.partial_rows(xc, chunk_twice[0]).astype(F64)
        rows[:, chunk_twice[1]] *= 2
        mean, rstd = I.finalize(rows, xc.shape[1] * xc.shape[2], eps)
    call["stats"] = UO.Rec(np.stack([q32(mean), q32(rstd)], -1), "f32")
    kw = dict(skip=residual) if L.skip_grad else dict(residual=residual)
    call["y"] = padded(q(I.forward(xc, P[L.name + "_g"], P[L.name + "_beta"], eps, L.act, L.leak, **kw)[0]), name)
    return call


def host_backward(L, P, fwd, dy, name, addend=None, add=True, exact=False):
    """What a correct device stores for the backward call of `fwd` (host_forward's record) -> (call, grads).  add=False leaves
    the addend out of dx although the call was handed one."""
    q = (lambda a: np.asarray(a, F64)) if exact else (lambda a: I.to_storage(a, name))
    x, xc = fwd["x"].f64[..., :L.cin], fwd["xc"].f64[..., :L.cout]
    call = dict(x=fwd["x"], xc=fwd["xc"], stats=fwd["stats"], y=fwd["y"] if L.skip_grad else None, dy=padded(dy, name),
                addend=None if addend is None else padded(addend, name), drop=None, param_grads=True, bwd_stats_chunks=0, dx=None, dskip=None,
                partial=None, next=None)
    grads = {}
    if L.norm:
        st = fwd["stats"].f64
        gs = dy * (UO.act_slope_from_output(fwd["y"].f64[..., :L.cout], L) if L.skip_grad else
                   I.slope(I.backward(dy, xc, P[L.name + "_g"], P[L.name + "_beta"], st[..., 0], st[..., 1], L.act, L.leak)["pre"], L.act, L.leak))
        o = I.backward(gs, xc, P[L.name + "_g"], P[L.name + "_beta"], st[..., 0], st[..., 1])
        dxc = q(o["dx"])
        grads.update(dgamma=o["dgamma"], dbeta=o["dbeta"])
        if L.skip_grad:
            call["dskip"] = padded(q(o["dskip"]), name)
    else:
        dxc = q(dy * UO.act_slope_from_output(xc, L))
    r = UO.conv_backward(L, x, P[L.name + "_w"], P[L.name + "_b"], dxc, np.zeros_like(dxc))
    call["dx"] = padded(q(r["dx"] + (addend if addend is not None and add else 0.0)), name)
    grads.update(dw=r["dw"], db=r["db"] if not L.norm else np.zeros(L.cout))
    return call, grads


def ok(stages):
    return all(s.ratio <= 1.0 and s.kinks <= UO.KINK_FRACTION for s in stages)


TINY = {
    "conv": UO.Layer("t", "conv", 1, "VALID", 1, True, UO.RELU, 0.0, 3, 5, 6, False, None),
    "conv_s2_same": UO.Layer("t", "conv", 2, "SAME", 0, True, UO.LRELU, 0.3, 3, 5, 6, False, None),
    "conv_valid_s2": UO.Layer("t", "conv", 2, "VALID", 0, True, UO.LRELU, 0.3, 3, 5, 6, False, None),
    "conv_no_norm_lrelu": UO.Layer("t", "conv", 2, "SAME", 0, False, UO.LRELU, 0.3, 3, 3, 6, False, None),
    "conv_no_norm_tanh": UO.Layer("t", "conv", 1, "VALID", 3, False, UO.TANH, 0.0, 7, 4, 3, False, None),
    "deconv_s2": UO.Layer("t", "deconv", 2, "VALID", 0, True, UO.RELU, 0.0, 3, 6, 5, False, None),
    "deconv_s1_no_norm": UO.Layer("t", "deconv", 1, "SAME", 0, False, UO.TANH, 0.0, 3, 6, 3, False, None),
    "residual": UO.Layer("t", "conv", 1, "VALID", 1, True, UO.NONE, 0.0, 3, 6, 6, False, None),
    "skip_grad": UO.Layer("t", "deconv", 1, "SAME", 0, True, UO.RELU, 0.0, 3, 6, 5, True, None),
}


# ---------------------------------------------------------------------------- (2) finite differences
@pytest.mark.parametrize("kind", list(TINY))
def test_the_bound_pass_states_the_same_layer(kind):
    """The float32 torch pass behind the sums of absolute terms is the oracle's layer: same values, same gradients."""
    L = TINY[kind]
    rng = np.random.default_rng([6, len(kind)])
    P = params(L, 4)
    x = np.abs(rng.standard_normal((2, 7, 9, L.cin)))
    w, b = np.abs(P["t_w"]), np.abs(P["t_b"])
    y = np.concatenate([UO._conv_tape(L, x[n:n + 1], w, b)[4].v for n in range(2)])
    assert np.allclose(UO._abs_conv(L, x, w, b), y, rtol=1e-4, atol=1e-5)
    cots = np.abs(rng.standard_normal(y.shape)), np.abs(rng.standard_normal(y.shape))       # one for x, one for w and b
    want = []
    for cot in cots:
        tape, vx, vw, vb, vy = UO._conv_tape(L, x, w, b)
        tape.backward([(vy, cot)])
        want.append((vx.g, vw.g, vb.g))
    for got, ref in zip(UO._abs_conv(L, x, w, b, cots), (want[0][0], want[1][1], want[1][2])):
        assert np.allclose(got, ref, rtol=1e-4, atol=1e-5)


def test_accumulation_terms_are_counted_per_gradient():
    """dx is bounded with R*S*K terms and dw / db with N*Ho*Wo: with an exact cotangent the bounds are those counts times 2^-24 times
    the sums of absolute terms (plus the final f32 store of dw / db), neither inflated by the other's count."""
    L = TINY["conv_valid_s2"]
    rng = np.random.default_rng(3)
    P = params(L, 5)
    x = rng.standard_normal((1, 9, 11, L.cin))
    Ho, Wo = UO.out_hw(L, 9, 11)
    dxc = rng.standard_normal((1, Ho, Wo, L.cout))
    r = UO.conv_backward(L, x, P["t_w"], P["t_b"], dxc, np.zeros_like(dxc))
    tape, vx, vw, vb, vy = UO._conv_tape(L, np.abs(x), np.abs(P["t_w"]), np.abs(P["t_b"]))
    tape.backward([(vy, np.abs(dxc))])
    Tx, Tw = 9 * L.cout, Ho * Wo
    assert Tx != Tw
    assert np.allclose(r["bdx"], Tx * UO.U32 * vx.g, rtol=1e-3) and np.allclose(r["bdw"] - UO.U32 * np.abs(r["dw"]), Tw * UO.U32 * vw.g, rtol=1e-3)


@pytest.mark.parametrize("kind", list(TINY))
def test_reference_matches_finite_differences(kind):
    L = TINY[kind]
    rng = np.random.default_rng([5, len(kind)])
    N, H, W = 2, 7, 9
    P = params(L, 1)
    x = rng.standard_normal((N, H, W, L.cin))
    Ho, Wo = UO.out_hw(L, H, W)
    res = rng.standard_normal((N, Ho, Wo, L.cout)) if kind in ("residual", "skip_grad") else None
    dy = rng.standard_normal((N, Ho, Wo, L.cout))

    def f(P_, x_, res_):
        c = host_forward(L, P_, x_, "f32", res_, exact=True)
        out = c["y"] if L.norm else c["xc"]
        return float((out.f64[..., :L.cout] * dy).sum())

    fwd = host_forward(L, P, x, "f32", res, exact=True)
    call, _ = host_backward(L, P, fwd, dy, "f32", exact=True)
    refs = {}
    _, parts = UO.check_backward(L, P, call, refs=refs)
    grads = {L.name + "_w": parts["dw"][0], "x": refs["dx"]}
    if L.norm:
        grads.update({L.name + "_g": parts["dgamma"][0], L.name + "_beta": parts["dbeta"][0]})
    else:
        grads[L.name + "_b"] = parts["db"][0]
    if L.skip_grad:
        grads["res"] = refs["dskip"]
    h = 1e-5
    for key, g in grads.items():
        for _ in range(6):
            idx = tuple(int(rng.integers(0, s)) for s in g.shape)
            vals = []
            for sign in (1, -1):
                P2, x2, r2 = {k: v.copy() for k, v in P.items()}, x.copy(), None if res is None else res.copy()
                tgt = x2 if key == "x" else r2 if key == "res" else P2[key]
                tgt[idx] += sign * h
                vals.append(f(P2, x2, r2))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - g[idx]) <= 1e-5 * (1 + abs(fd)), (kind, key, idx, fd, g[idx])


# ---------------------------------------------------------------------------- (3) sensitivity
SENS = UO.Layer("t", "conv", 1, "VALID", 1, True, UO.RELU, 0.0, 3, 16, 16, False, None)


def _sens_inputs(seed=0):
    rng = np.random.default_rng([9, seed])
    N, H, W = 2, 6, 8
    P = UO.quantised_params(params(SENS, seed, scale=0.1), "bf16")
    x = I.to_storage(rng.standard_normal((N, H, W, SENS.cin)), "bf16")
    res = I.to_storage(rng.standard_normal((N, H, W, SENS.cout)), "bf16")
    dy = I.to_storage(rng.standard_normal((N, H, W, SENS.cout)), "bf16")
    add = I.to_storage(rng.standard_normal((N, H, W, SENS.cin)), "bf16")
    return P, x, res, dy, add


def test_a_correct_result_rounded_to_storage_passes():
    for L in list(TINY.values()) + [SENS]:
        for name in ("bf16", "f32"):
            rng = np.random.default_rng([11, L.R, L.cin])
            P = UO.quantised_params(params(L, 2), name)
            x = I.to_storage(rng.standard_normal((2, 7, 9, L.cin)), name)
            Ho, Wo = UO.out_hw(L, 7, 9)
            res = I.to_storage(rng.standard_normal((2, Ho, Wo, L.cout)), name) if L.norm else None
            dy = I.to_storage(rng.standard_normal((2, Ho, Wo, L.cout)), name)
            add = I.to_storage(rng.standard_normal(x.shape), name) if not L.skip_grad else None
            fwd = host_forward(L, P, x, name, res)
            assert ok(UO.check_forward(L, P, fwd)), (L, name, UO.worst(UO.check_forward(L, P, fwd)))
            call, grads = host_backward(L, P, fwd, dy, name, add)
            stages, parts = UO.check_backward(L, P, call)
            stages += UO.check_param_grads(L, [parts], {k: np.asarray(v, np.float32) for k, v in grads.items()})
            assert ok(stages), (L, name, UO.worst(stages))


def test_a_border_row_replaced_by_its_neighbour_fails():
    P, x, res, dy, add = _sens_inputs()
    fwd = host_forward(SENS, P, x, "bf16", res)
    assert ok(UO.check_forward(SENS, P, fwd))
    fwd["xc"].a[:, 0] = fwd["xc"].a[:, 1]
    bad = [s for s in UO.check_forward(SENS, P, fwd) if s.ratio > 1]
    assert bad and bad[0].stage == "xc" and bad[0].index[1] == 0
    call, _ = host_backward(SENS, P, host_forward(SENS, P, x, "bf16", res), dy, "bf16", add)
    assert ok(UO.check_backward(SENS, P, call)[0])
    call["dx"].a[:, -1] = call["dx"].a[:, -2]
    assert [s.stage for s in UO.check_backward(SENS, P, call)[0] if s.ratio > 1] == ["dx"]


def test_a_dropped_tap_fails():
    P, x, res, dy, add = _sens_inputs()
    Pbad = dict(P)
    Pbad["t_w"] = P["t_w"].copy()
    Pbad["t_w"][0, 2] = 0.0
    fwd = host_forward(SENS, Pbad, x, "bf16", res)
    assert [s.stage for s in UO.check_forward(SENS, P, fwd) if s.ratio > 1] == ["xc"]
    good = host_forward(SENS, P, x, "bf16", res)
    call, grads = host_backward(SENS, Pbad, good, dy, "bf16", add)              # the data gradient without the tap
    stages, parts = UO.check_backward(SENS, P, call)
    assert [s.stage for s in stages if s.ratio > 1] == ["dx"]
    call, grads = host_backward(SENS, P, good, dy, "bf16", add)                 # the weight gradient of the tap left at 0
    grads["dw"] = grads["dw"].copy()
    grads["dw"][0, 2] = 0.0
    stages, parts = UO.check_backward(SENS, P, call)
    assert ok(stages)
    assert [s.stage for s in UO.check_param_grads(SENS, [parts], grads) if s.ratio > 1] == ["dw"]


def test_a_statistics_chunk_counted_twice_fails():
    P, x, res, dy, add = _sens_inputs()
    assert ok(UO.check_forward(SENS, P, host_forward(SENS, P, x, "bf16", res, chunk_twice=None)))
    fwd = host_forward(SENS, P, x, "bf16", res, chunk_twice=(6, 2))
    bad = {s.stage for s in UO.check_forward(SENS, P, fwd) if s.ratio > 1}
    assert {"mean", "rstd"} <= bad


def test_the_addend_left_out_fails():
    P, x, res, dy, add = _sens_inputs()
    fwd = host_forward(SENS, P, x, "bf16", res)
    call, _ = host_backward(SENS, P, fwd, dy, "bf16", add, add=False)
    assert [s.stage for s in UO.check_backward(SENS, P, call)[0] if s.ratio > 1] == ["dx"]


def test_swapped_weights_in_the_second_half_fail():
    Pa, x, res, dy, add = _sens_inputs(0)
    Pb = UO.quantised_params(params(SENS, 3, scale=0.1), "bf16")
    # a stacked batch: images 0, 1 belong to network a, images 2, 3 to network b; the stand-in convolves all four with a's kernels
    xs, rs = np.concatenate([x, x[::-1]]), np.concatenate([res, res])
    right = [host_forward(SENS, P, xs[sl], "bf16", rs[sl]) for P, sl in ((Pa, slice(0, 2)), (Pb, slice(2, 4)))]
    wrong = host_forward(SENS, dict(Pb, t_w=Pa["t_w"]), xs[2:], "bf16", rs[2:])
    assert ok(UO.check_forward(SENS, Pa, right[0])) and ok(UO.check_forward(SENS, Pb, right[1]))
    assert [s.stage for s in UO.check_forward(SENS, Pb, wrong) if s.ratio > 1] == ["xc"]


# ---------------------------------------------------------------------------- the recorder, on a stand-in walk
def test_recorder_copies_at_call_time_restores_and_knows_its_records():
    import torch
    from types import SimpleNamespace
    from tests import unit_spy

    class Store:
        grad = torch.zeros(1)

        def export(self, buf=None):
            return {"t_w": np.zeros(1)}

    class FakeUnit:
        name, norm, skip_grad, drop_layer = "t", True, False, None
        net = SimpleNamespace(P=Store(), eps=1e-3)

        def forward(self, x, residual=None, record_only=False, out=None, drop=None):
            xc = x * 2
            return xc + 1, (SimpleNamespace(stats_chunks=0, bwd_stats_chunks=0), x, xc, torch.zeros(1, 8, 2))

        def backward(self, rec, dy, want_dx=True, param_grads=True, gbuf=None, addend=None, dy_partial=None, next_norm=None):
            return dy * 2

    ua, ub = FakeUnit(), FakeUnit()
    walk = SimpleNamespace(conv_units=lambda: [ua, ub])
    x = torch.ones(1, 2, 2, 8)
    with unit_spy.Spy(walk) as spy:
        y, ra = ua.forward(x)
        _, rb = ub.forward(y)
        x.zero_()                                        # (a reused buffer: the recorded copy must not follow)
        ub.backward(rb, torch.ones(1, 2, 2, 8))
        ua.backward(rb, torch.ones(1, 2, 2, 8))         # the wrong record
    assert "forward" not in vars(ua) and "backward" not in vars(ub)
    kinds = [(k, u is ua, c.get("own_record")) for k, u, c in spy.calls]
    assert kinds == [("forward", True, None), ("forward", False, None), ("backward", False, True), ("backward", True, False)]
    assert spy.calls[0][2]["x"].a.min() == 1.0 and spy.calls[0][2]["xc"].name == "f32" and spy.calls[2][2]["dx"].a.max() == 2.0


def test_the_second_rounding_is_granted_on_the_fold_band_of_the_narrow_routes_only():
    """A 7x7 REFLECT layer without a norm, bf16, no addend.  A stand-in that stores bf16(dx_zero), adds the mirrored terms and rounds
    again passes where the route is a narrow one; the band is what include/sggan.h names; with an addend, or on another route, the
    bound is that of one rounding."""
    L = TINY["conv_no_norm_tanh"]
    rng = np.random.default_rng(12)
    P = UO.quantised_params(params(L, 6, scale=0.1), "bf16")
    q = lambda a: I.to_storage(a, "bf16")
    x = q(rng.standard_normal((1, 12, 14, L.cin)))
    fwd = host_forward(L, P, x, "bf16")
    dy = q(rng.standard_normal((1, 12, 14, L.cout)))
    call, _ = host_backward(L, P, fwd, dy, "bf16")
    dxc = q(dy * UO.act_slope_from_output(fwd["xc"].f64[..., :L.cout], L))
    ref = UO.conv_backward(L, x, P["t_w"], P["t_b"], dxc, np.zeros_like(dxc))["dx"]
    zero = UO.conv_backward(L._replace(reflect=0, padding="SAME"), x, P["t_w"], P["t_b"], dxc, np.zeros_like(dxc))["dx"]
    mirrored = ref - zero
    reached = np.abs(mirrored).max(axis=(0, 3)) > 0
    rows = np.zeros(12, bool); rows[1:4] = True; rows[8:11] = True
    cols = np.zeros(14, bool); cols[1:4] = True; cols[10:13] = True
    assert np.array_equal(reached, rows[:, None] | cols[None, :])
    call["dx"] = padded(q(q(zero) + mirrored), "bf16")
    assert ok(UO.check_backward(L, P, dict(call, dgrad_route="HALO_NARROW_IN"))[0])
    once = UO.check_backward(L, P, dict(call, dgrad_route="N7"))[0]
    twice = UO.check_backward(L, P, dict(call, dgrad_route="HALO_DGRAD_NARROW"))[0]
    b1, b2 = [next(s for s in st if s.stage == "dx") for st in (once, twice)]
    assert b2.ratio <= 1.0 and b1.ratio >= b2.ratio
