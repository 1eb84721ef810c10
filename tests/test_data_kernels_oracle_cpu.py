"""tests/data_kernels_oracle.py without a GPU.  For every case tests/test_gpu_data_kernels.py uses:

* the float32 statement of the kernels' arithmetic equals an exact evaluation in integers before the one allowed rounding (the
  division by 255.0f), so the GPU comparison can be for equality;
* the oracle agrees with the package's own host statements, data.apply_tables and data.apply_augment, to 1e-6;
* the launch plan, restated from the kernels' documented formulas, selects the path the case is named for (rq class, refusal,
  ragged tiles, tail chunks, alignment residues, window class).

A construction that fails here is redesigned here."""
import itertools
from fractions import Fraction

import numpy as np
import pytest
import torch

from sggan_amd import data as D
from tests import data_kernels_oracle as O

AGREE = 1e-6
F32 = np.float32


# ---------------------------------------------------------------------------- tables
@pytest.mark.parametrize("name", list(O.CASES))
def test_tables_are_sixteenths_with_zeros_and_the_promised_starts(name):
    c, src, rows, cols = O.build(name)
    for (w16, starts, step), taps, n_in, n_out in ((rows, c["TR"], c["H0"], c["H"]), (cols, c["TC"], c["W0"], c["W"])):
        assert w16.shape == (n_out, taps) and (w16 >= 0).all() and (w16.sum(axis=1) == 16).all()
        w32 = O.kernel_table((w16, starts, step))[0]
        assert w32.dtype == F32 and np.array_equal(w32.astype(np.float64) * 16, w16)          # k/16 exactly, rows sum to exactly 1
        assert all(sum(Fraction(float(v)) for v in r) == 1 for r in w32[:3])
        d = np.diff(starts.astype(np.int64))
        assert starts.dtype == np.int32 and starts[0] >= 0 and (d >= 0).all() and (starts + taps <= n_in).all()
        assert step == (int(d.max()) if n_out > 1 else 0)
        if taps >= 3 and n_out >= 4:                              # zero weights at both ends of a row and inside one
            assert (w16[:, 0] == 0).any() and (w16[:, -1] == 0).any() and (w16[:, 1:-1] == 0).any()
        if taps >= 2 and n_out >= 4:
            assert (w16[:, -1] > 0).any() and (w16[:, 0] > 0).any()            # ... and outermost taps that carry weight
    assert src.nbytes == c["nbytes"] < O.SOURCE_LIMIT


# ---------------------------------------------------------------------------- resample: exactness and agreement
@pytest.mark.parametrize("name", list(O.CASES))
def test_resample_float32_statement_is_exact_and_agrees_with_apply_tables(name):
    c, src, rows, cols = O.build(name)
    acc = O.resample_int(name)                                   # exact, in integers
    stmt = O.resample_f32_statement(name)                         # float32, the kernels' order
    scale = 256 if c["kind"] == "u8" else 65536
    assert stmt.dtype == F32 and np.array_equal(stmt.astype(np.float64) * scale, acc)         # no rounding anywhere before the division
    assert acc.min() >= 0 and acc.max() <= (255 * 256 if c["kind"] == "u8" else 65536) < 2 ** 24
    v = O.resample_values(name)
    if c["kind"] == "u8":                                         # one rounding: the correctly rounded quotient of the exact sum
        q = acc.astype(np.float64) / 256.0 / 255.0                # within 2^-53 of the true quotient; v is its nearest float32
        assert np.abs(v.astype(np.float64) - q).max() <= 2.0 ** -25
        flat, vf = acc.reshape(-1), v.reshape(-1)
        for k in np.linspace(0, flat.size - 1, 25).astype(int):   # and exactly so, in rationals, on a sample of elements
            x = Fraction(int(flat[k]), 256 * 255)
            lo, hi = np.nextafter(vf[k], F32(-1)), np.nextafter(vf[k], F32(2))
            assert abs(Fraction(float(vf[k])) - x) <= min(abs(Fraction(float(lo)) - x), abs(Fraction(float(hi)) - x))
    else:
        assert np.array_equal(v.astype(np.float64) * 65536, acc)
    rt, ct = O.kernel_table(rows), O.kernel_table(cols)
    for m in range(c["M"]):
        want = D.apply_tables(src[m], rt, ct)
        assert np.abs(v[m].astype(np.float64) - want).max() <= AGREE
    # what the GPU test compares with: channel selection, flip, zero padding, bf16 = RNE of the float32 value
    C = c["C"][-1]
    e32, e16 = O.resample_expect(name, C), O.resample_expect(name, C, bf16=True)
    assert e32.shape == (len(c["index"]), c["H"], c["W"], 8) and not e32[..., C:].any()
    for n, (i, f) in enumerate(zip(c["index"], c["flip"])):
        assert np.array_equal(e32[n, :, ::-1, :C] if f else e32[n, ..., :C], v[i][..., :C])
    assert np.array_equal(e16, torch.as_tensor(e32).to(torch.bfloat16).float().numpy())


# ---------------------------------------------------------------------------- resample: the path each case selects
def test_case_combinations_cover_what_the_issue_lists():
    u8 = [O.CASES[n] for n in O.names("u8")]
    assert {c["Cs"] for c in u8} == {3, 4} and {c["M"] for c in u8} >= {1, 2, 3}
    for Cs in (3, 4):
        assert {C for c in u8 if c["Cs"] == Cs for C in c["C"]} == set(range(1, Cs + 1))
    for c in O.CASES.values():
        assert max(c["index"]) == c["M"] - 1 and len(c["index"]) == len(c["flip"])
        if c["kind"] == "u8" and c["M"] > 1:
            assert len(set(c["index"])) < len(c["index"]) and c["index"] != sorted(c["index"])     # repeated, out of order
        if len(c["flip"]) > 1:
            assert set(c["flip"]) == {0, 1}                                                          # mixed flips
    assert {C for n in O.names("f32") for C in O.CASES[n]["C"]} == {1, 2, 3, 4}


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_tail_grid_reaches_every_tile_and_chunk_edge(kind):
    cases = [O.CASES[n] for n in O.names(kind, "tail-")]
    assert {(c["H"], c["W"]) for c in cases} == set(itertools.product(O.TAIL_H, O.TAIL_W))
    assert {c["TR"] for c in cases} == set(O.TAIL_TR) and {c["TC"] for c in cases} == set(O.TAIL_TC)
    assert {c["rstep"] for c in cases} == set(O.TAIL_RSTEP) and {O.build(c["name"])[3][2] for c in cases} >= {0, 1, 2, 3}
    plans = {c["name"]: O.plan_of(c["name"]) for c in cases}
    assert not any(p["refused"] for p in plans.values())
    assert {p["wstride"] for p in plans.values()} == {64, 128, 256}
    for W in O.TAIL_W:                                            # every W meets both tap counts' weight tiles through its wstride class
        assert {plans[c["name"]]["wstride"] for c in cases if c["W"] == W} == {min(-(-W // 64) * 64, 256)}
    tail_chunk = [c["name"] for c in cases if any(ch[-1] < plans[c["name"]]["rq"] and len(ch) > 1 for ch in plans[c["name"]]["chunks"])]
    overlap = [c["name"] for c in cases if any(b1[0] < b0[1] for b0, b1 in zip(plans[c["name"]]["bands"], plans[c["name"]]["bands"][1:]))]
    print(f"{kind}: {len(tail_chunk)} cases with a band that is no multiple of rq, {len(overlap)} with overlapping bands of neighbouring row blocks")
    assert len(tail_chunk) >= 8 and len(overlap) >= 4
    ragged_cols = [c for c in cases if c["W"] % 256 and c["W"] > 256]
    assert ragged_cols and all(len(plans[c["name"]]["tiles"]) == -(-c["W"] // 256) for c in ragged_cols)


@pytest.mark.parametrize("name", O.names("u8", "rq-") + O.names("f32", "rq-"))
def test_rq_cases_select_their_class(name):
    c, p = O.CASES[name], O.plan_of(name)
    assert c["W"] == 256 and p["wstride"] == 256 and p["wbytes"] == 1024 * c["TC"]
    assert O.build(name)[3][2] == c["cstep"] and p["span_cap"] == 255 * c["cstep"] + c["TC"] <= c["W0"]
    if c["expect"] == "refused":
        assert p["refused"] and p["wbytes"] + p["seg"] > 65536
    else:
        assert not p["refused"] and p["rq"] == c["expect"]
        if 1 < p["rq"]:
            assert any(ch[-1] < p["rq"] for ch in p["chunks"])    # a tail chunk with nq < rq
    print(name, {k: p[k] for k in ("wbytes", "span_cap", "seg", "rq", "refused")})


def test_rq_classes_are_all_present():
    for Cs in (3, 4):
        got = {O.CASES[n]["expect"] for n in O.names("u8", f"rq-u8-Cs{Cs}")}
        assert {8, 1, "refused"} <= got and any(isinstance(v, int) and 1 < v < 8 for v in got), got
    assert {O.CASES[n]["expect"] for n in O.names("u8", "rq-u8-Cs4")} == {8, 7, 3, 1, "refused"}       # the issue's own values
    assert {O.CASES[n]["expect"] for n in O.names("f32", "rq-")} == {8, 3, 1, "refused"}


@pytest.mark.parametrize("name", O.names("u8", "align-") + O.names("u8", "single-"))
def test_alignment_cases_reach_every_residue_and_both_buffer_ends(name):
    """With the flat buffer's base 16-byte aligned (the GPU test asserts it), the absolute address of a staged row's first byte is
    off + ((m * H0 + r) * W0 + x_lo) * Cs."""
    c, p = O.CASES[name], O.plan_of(name)
    off = c["off"] or 0
    assert len(p["tiles"]) == 1 and p["tiles"][0][0] == 0
    staged = sorted({r for lo, hi in p["bands"] for r in range(lo, hi)})
    assert staged == list(range(c["H0"])) and set(c["index"]) == set(range(c["M"]))              # every row of every image is staged
    res = {(off + (m * c["H0"] + r) * c["W0"] * c["Cs"]) % 16 for m in range(c["M"]) for r in staged}
    if name.startswith("align-"):
        assert c["W0"] % 2 == 1 and res == (set(range(16)) if c["Cs"] == 3 else {0, 4, 8, 12})
    if c["off"] is not None:
        assert off % 16 != 0                                     # first row of the first image: its first piece starts before the view (g < 0)
    assert (off + c["nbytes"]) % 16 != 0                          # the last row's last piece straddles the end of the buffer
    if name.startswith("single-"):
        assert c["nbytes"] == c["Cs"] and (c["H0"], c["W0"], c["H"], c["W"], c["TR"], c["TC"], c["M"]) == (1,) * 7
        assert O.resample_values(name).min() > 0                 # the one pixel is no zero: a result that was never summed shows
    if c["Cs"] == 4:
        assert off % 4 == 0


def test_degenerate_cases_are_degenerate():
    c, p = O.CASES["degen-colstep0-TC=W0"], O.plan_of("degen-colstep0-TC=W0")
    cols = O.build(c["name"])[3]
    assert cols[2] == 0 and c["TC"] == c["W0"] and not cols[1].any() and p["span_cap"] == c["W0"] and p["wstride"] == 128
    c, p = O.CASES["degen-TR=H0"], O.plan_of("degen-TR=H0")
    assert c["TR"] == c["H0"] and not O.build(c["name"])[2][1].any() and all(b == (0, c["H0"]) for b in p["bands"])
    c, p = O.CASES["degen-span-clamped-by-W0"], O.plan_of("degen-span-clamped-by-W0")
    assert p["span_formula"] > c["W0"] == p["span_cap"] and O.build(c["name"])[3][1][-1] == c["W0"] - c["TC"]
    c = O.CASES["degen-last-starts-at-the-end"]
    _, _, rows, cols = O.build(c["name"])
    assert rows[1][-1] == c["H0"] - c["TR"] and cols[1][-1] == c["W0"] - c["TC"] and len(O.plan_of(c["name"])["tiles"]) == 2
    c = O.CASES["degen-f32-colstep0-TR=H0"]
    assert c["TR"] == c["H0"] and c["TC"] == c["W0"]
    for n in O.names("u8", "flip-") + O.names("f32", "flip-"):
        assert O.CASES[n]["W"] == 257 and O.plan_of(n)["tiles"][1][1] == O.CASES[n]["TC"] and set(O.CASES[n]["flip"]) == {0, 1}


# ---------------------------------------------------------------------------- warp
def _ident_rows(S):
    return np.ones((S, 1), F32), np.arange(S, dtype=np.int32), 1


@pytest.mark.parametrize("which", O.WARP_TABLES)
@pytest.mark.parametrize("S", O.WARP_S)
def test_warp_statement_is_exact_and_agrees_with_apply_augment(S, which):
    groups = O.warp_groups(S)
    for Cs in (3, 4):
        src, tab = O.warp_source(S, Cs, which)
        assert src.shape == (2, S, {O.WARP_TABLES[0]: S, O.WARP_TABLES[1]: 2 * S, O.WARP_TABLES[2]: 3 * S + 1}[which], Cs)
        assert (tab[0].sum(axis=1) == 16).all() and tab[1][-1] + tab[0].shape[1] == src.shape[2]
        for img in src:
            hint = O.squared_int(img, tab)
            stmt = O.band_f32(img[..., :3].astype(F32), tab, 1)
            assert np.array_equal(stmt.astype(np.float64) * 16, hint) and hint.max() <= 255 * 16        # exact before the one division
            A32 = O.squared_f32(img, tab)
            A64 = D.apply_tables(img[..., :3], _ident_rows(S), O.kernel_table(tab))
            assert A32.dtype == F32 and np.abs(A32 - A64).max() <= 2.0 ** -24
            if Cs == 4:
                continue
            for name, m in itertools.chain.from_iterable(groups.values()):
                got = O.warp_expect(A32, m)
                assert got.dtype == F32 and not got[..., 3].any()
                assert np.abs(got[..., :3] - D.apply_augment(A64, m)).max() <= AGREE, name
                assert np.array_equal(O.warp_points(m, S)[0], D.augment_inside(m, S))


@pytest.mark.parametrize("S", O.WARP_S)
def test_warp_maps_are_dyadic_and_their_weights_powers_of_two(S):
    py, px = np.meshgrid(2 * np.arange(S) + 1, 2 * np.arange(S) + 1, indexing="ij")         # 2 * (pixel centre), integers
    rng = np.random.default_rng(S)
    a = (rng.integers(0, 255 * 16 + 1, (S, S)).astype(F32) / F32(16)) / F32(255)             # any window pixel
    for name, m in itertools.chain.from_iterable(O.warp_groups(S).values()):
        m4 = m * 4
        assert np.array_equal(m4, np.rint(m4)) and np.abs(m4).max() < 2 ** 20, name           # entries are multiples of 1/4
        mi = m4.astype(np.int64)
        inside, u, v = O.warp_points(m, S)
        # 8 * coordinate in integers: (4 m0)(2 px) + (4 m1)(2 py) + 8 m2 -- the float64 evaluation carries no rounding at all
        for coord, row, shift in ((u, mi[1, 0], 4), (v, mi[1, 1], 4)):
            exact = row[0] * px + row[1] * py + 2 * row[2] - shift
            assert np.array_equal(coord * 8, exact), name
            assert set(np.unique(exact % 8)) <= {0, 4}, name                                  # fractions 0 or 1/2 only
        fx8 = mi[0, 0, 0] * px + mi[0, 0, 1] * py + 2 * mi[0, 0, 2]
        fy8 = mi[0, 1, 0] * px + mi[0, 1, 1] * py + 2 * mi[0, 1, 2]
        assert np.array_equal(inside, (fx8 >= 0) & (fx8 <= 8 * S) & (fy8 >= 0) & (fy8 <= 8 * S)), name
        _, _, ws = O.warp_neighbours(m, S)
        tot = np.zeros((S, S))
        for w in ws:
            assert set(np.unique(w)) <= {0.0, 0.25, 0.5, 1.0}, name
            p32 = w * a
            assert p32.dtype == F32 and np.array_equal(p32.astype(np.float64), w.astype(np.float64) * a.astype(np.float64))   # exact product
            tot += w
        assert np.array_equal(tot, np.ones((S, S)))


@pytest.mark.parametrize("S", O.WARP_S)
def test_warp_cases_select_their_window_class(S):
    g = O.warp_groups(S)
    named = {n: m for ms in g.values() for n, m in ms}
    plans = {}
    for group, ms in g.items():
        assert len(ms) >= 2                                       # several samples with different matrices in one launch
        mats = np.stack([m for _, m in ms])
        win = D.warp_window(mats)
        plans[group] = p = O.warp_plan(mats, S, win)
        assert not p["refused"] and p["covered"], (group, p)      # the window holds every neighbour: warp_expect is what the kernel owes
        print(f"S={S} {group}: window {win} -> {p['wh']}x{p['ww']}, {p['lds']} B, {p['outside_tiles']} of {p['tiles']} tiles wholly outside, {len(p['origins'])} origins")
    assert D.warp_window(np.stack([m for _, m in g["unit"]])) == (19, 67)
    assert D.warp_window(np.stack([m for _, m in g["double"]])) == (34, 130) and plans["double"]["cols_clamped"] and plans["double"]["ww"] == S
    assert D.warp_window(np.stack([m for _, m in g["swap"]])) == (67, 19) and plans["swap"]["wh"] == min(S, 67)
    assert plans["swap"]["rows_clamped"] == (S < 67) and plans["swap"]["wh"] >= plans["swap"]["ww"]      # tall and narrow; clamped to S below 67
    one = lambda n, win=(19, 67): O.warp_plan(named[n][None], S, win)
    p = one("fill-all-outside")
    assert p["outside_tiles"] == p["tiles"] == -(-S // 16) * -(-S // 64)
    assert one("sample+2S")["origins"] == {(S - 1, S - 1)} and one("sample-2S")["origins"] == {(0, 0)}
    if S >= 48:
        assert one(f"translate{0:+}{S // 3:+}")["outside_tiles"] >= 1          # a tile of the zero-fill band lies wholly outside
    # every neighbour of sample+-2S is the last / first row and column
    for n, edge in (("sample+2S", S - 1), ("sample-2S", 0)):
        inside, idx, _ = O.warp_neighbours(named[n], S)
        assert inside.all() and all((a == edge).all() for a in idx)
    # what the named maps mean, stated on the oracle's own output
    src, tab = O.warp_source(S, 3, O.WARP_TABLES[2])
    A = O.squared_f32(src[0], tab)
    out = {n: O.warp_expect(A, named[n])[..., :3] for n in named}
    assert np.array_equal(out["identity"], A) and np.array_equal(out["flip-x"], A[:, ::-1]) and np.array_equal(out["flip-y"], A[::-1])
    assert np.array_equal(out["flip-xy"], A[::-1, ::-1]) and np.array_equal(out["swap"], A.transpose(1, 0, 2))
    assert not out["fill-all-outside"].any() and not out["fill-all-outside-y"].any()
    assert np.array_equal(out["sample+2S"], np.broadcast_to(A[-1, -1], A.shape)) and np.array_equal(out["sample-2S"], np.broadcast_to(A[0, 0], A.shape))
    assert not out["shift-x-1.0"][:, 0].any() and not out["shift-x+1.0"][:, -1].any()
    assert not out["shift-y-1.0"][0].any() and not out["shift-y+1.0"][-1].any()
    assert np.array_equal(out["shift-x-1.0"][:, 1:], A[:, :-1]) and np.array_equal(out["shift-x+1.0"][:, :-1], A[:, 1:])
    # a shift of exactly -1/2 / +1/2 keeps the first / last column inside (fx == 0 / fx == S) and replicates the edge there
    assert O.warp_points(named["shift-x-0.5"], S)[0].all() and O.warp_points(named["shift-x+0.5"], S)[0].all()
    assert np.array_equal(out["shift-x-0.5"][:, 0], A[:, 0]) and np.array_equal(out["shift-x+0.5"][:, -1], A[:, -1])
    T = S // 3
    if T:
        t = out[f"translate{T:+}{0:+}"]
        assert not t[:, S - T:].any() and np.array_equal(t[:, :S - T], A[:, T:])
    for n in ("half", "half-flip-x", "half-x-only"):              # crop-like: every sample stays inside, unclamped
        inside, u, v = O.warp_points(named[n], S)
        assert inside.all() and u.min() >= 0 and v.min() >= 0 and np.ceil(u).max() <= S - 1 and np.ceil(v).max() <= S - 1


def test_warp_lds_limit():
    g64, g65 = O.warp_groups(64), O.warp_groups(65)
    mats = np.stack([m for k in ("double", "swap", "half") for _, m in g64[k]] + [g64["unit"][0][1]])
    p = O.warp_plan(mats, 64, (64, 64))
    assert p["lds"] == 65536 and not p["refused"] and p["covered"]                    # exactly the budget: accepted
    p = O.warp_plan(np.stack([g65["unit"][0][1]]), 65, (65, 65))
    assert p["lds"] == 67600 and p["refused"]
