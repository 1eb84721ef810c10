"""Oracles and case tables for the input-pipeline kernels -- sgg_resample_u8, sgg_resample_f32 (csrc/resample.hip) and
sgg_warp_affine_u8 (csrc/warp.hip) -- at their tile, band and window edges.  Test infrastructure, written from include/sggan.h
and the kernels' header comments; the package never imports it and it does not import the package.

Everything here is EXACT by construction, so the GPU tests compare for equality:

* band tables are synthetic: weights k/16 whose rows sum to exactly 1 (zeros at the ends of a row and inside it), starts
  min(i * step, n_in - taps), step = max(diff(starts));
* resample_u8: uint8 sources make every horizontal sum a number <= 255 with 4 fractional bits and every vertical sum one with
  8, exact in float32 in any order; the oracle sums in integers (weights x 16, result x 256) and divides once by 255 in float32;
* resample_f32: sources k/256, no division, at most 16 fractional bits;
* warp: a window pixel is the horizontal sum / 255 (one rounding); matrices are dyadic with sample coordinates whose fractions
  are 0 or 1/2, so the bilinear weights are in {0, 1/4, 1/2, 1}, every fmaf is an exact product and one float32 addition, and
  np.float32 arithmetic in the kernel's order (w00 a00, + w01 a01, + w10 a10, + w11 a11) gives the same bits.

tests/test_data_kernels_oracle_cpu.py proves these premises for every case; the launch plans below restate the kernels'
documented formulas so that each named case can be shown to select the path its name claims."""
import functools
import itertools

import numpy as np

CPAD = 8
RS_RB, RS_RQ, RS_CB, RS_LDS = 8, 8, 256, 65536          # resample.hip: rows per block, rows per chunk, columns per block, LDS
WP_TH, WP_TW, WP_LDS = 16, 64, 65536                    # warp.hip: tile rows, tile columns, LDS
SOURCE_LIMIT = 200 * 1000                               # bytes: every source of this module stays below it
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------- band tables
def sixteenths(rng, n_out, taps):
    """(n_out, taps) int64 weights in sixteenths, every row summing to 16.  Row i has a zero first tap (i % 4 == 0), a zero last
    tap (1) or a zero middle tap (2) where taps allow it, and further zeros at random."""
    w = np.zeros((n_out, taps), np.int64)
    for i in range(n_out):
        live = rng.random(taps) < 0.7
        if taps > 1:
            live[-1] = True                                       # the outermost taps carry weight unless forced to zero below
            live[0] = True
            if i % 4 == 0:
                live[0] = False
            if i % 4 == 1:
                live[-1] = False
            if i % 4 == 2 and taps > 2:
                live[taps // 2] = False
        else:
            live[0] = True
        idx = np.flatnonzero(live)
        if len(idx) > 16:                                         # more live taps than sixteenths: keep the two outermost
            idx = np.concatenate([idx[[0, -1]], rng.choice(idx[1:-1], 14, replace=False)])
        w[i] = np.bincount(np.concatenate([idx, rng.choice(idx, 16 - len(idx))]), minlength=taps)   # every live tap >= 1/16
    assert (w.sum(axis=1) == 16).all()
    return w


def make_table(rng, n_in, n_out, taps, step):
    """(w16 int64 (n_out, taps), starts int32 (n_out,), step): starts = min(i * step, n_in - taps), step = max(diff(starts))."""
    assert 1 <= taps <= n_in
    starts = np.minimum(np.arange(n_out, dtype=np.int64) * step, n_in - taps).astype(np.int32)
    real = int(np.diff(starts).max()) if n_out > 1 else 0
    assert (np.diff(starts) >= 0).all() and starts[-1] + taps <= n_in
    return sixteenths(rng, n_out, taps), starts, real


def kernel_table(tab):
    """The table as the kernels take it: float32 weights k/16, int32 starts, step."""
    w16, starts, step = tab
    return (w16.astype(np.float64) / 16.0).astype(F32), starts, step


def band_int(x, tab, axis):
    """Exact: integer x reduced along `axis` by the table's integer weights (the result carries a factor 16)."""
    w16, starts, _ = tab
    x = np.moveaxis(np.asarray(x, np.int64), axis, 0)
    out = np.zeros((len(starts),) + x.shape[1:], np.int64)
    for k in range(w16.shape[1]):
        out += w16[:, k].reshape((-1,) + (1,) * (x.ndim - 1)) * x[starts.astype(np.int64) + k]
    return np.moveaxis(out, 0, axis)


def band_f32(x, tab, axis):
    """The kernels' float32 statement of one pass: taps ascending, acc = fl(fl(w * x) + acc) (the product is exact here, so this is
    the fmaf)."""
    w, starts, _ = kernel_table(tab)
    x = np.moveaxis(np.asarray(x, F32), axis, 0)
    out = np.zeros((len(starts),) + x.shape[1:], F32)
    for k in range(w.shape[1]):
        out = w[:, k].reshape((-1,) + (1,) * (x.ndim - 1)) * x[starts.astype(np.int64) + k] + out
    assert out.dtype == F32
    return np.moveaxis(out, 0, axis)


def bf16_rne(x):
    """float32 -> the float32 value of its bf16 rounding (nearest, ties to even); finite input."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(F32)


# ---------------------------------------------------------------------------------------------------------- resample: plan
def resample_plan(kind, H0, W0, H, W, TR, TC, cstep, Cs, rs, cs):
    """The launch plan of sgg_resample_u8 / _f32 restated from the documented formulas, and what each block then walks:
    bands[b] = (r_lo, r_hi) source rows of row block b, chunks[b] = the staged row counts, tiles[t] = (x_lo, span)."""
    wcols = min(W, RS_CB)
    wstride = -(-wcols // 64) * 64
    wbytes = 4 * TC * wstride
    span_formula = (wcols - 1) * cstep + TC
    span_cap = min(span_formula, W0)
    seg = ((span_cap * Cs + 30) // 16) * 16 if kind == "u8" else 16 * span_cap
    refused = wbytes + seg > RS_LDS
    p = dict(wstride=wstride, wbytes=wbytes, span_formula=span_formula, span_cap=span_cap, seg=seg, refused=refused, rq=None)
    if refused:
        return p
    p["rq"] = rq = min(RS_RQ, (RS_LDS - wbytes) // seg)
    p["bands"], p["chunks"], p["tiles"] = [], [], []
    for i0 in range(0, H, RS_RB):
        nrow = min(RS_RB, H - i0)
        r_lo, r_hi = int(rs[i0]), min(int(rs[i0 + nrow - 1]) + TR, H0)
        p["bands"].append((r_lo, r_hi))
        p["chunks"].append([min(rq, r_hi - rb) for rb in range(r_lo, r_hi, rq)])
    for j0 in range(0, W, RS_CB):
        ncol = min(RS_CB, W - j0)
        x_lo, x_hi = int(cs[j0]), min(int(cs[j0 + ncol - 1]) + TC, W0)
        assert x_hi - x_lo <= span_cap
        p["tiles"].append((x_lo, x_hi - x_lo))
    return p


# ---------------------------------------------------------------------------------------------------------- resample: cases
def _case(name, kind, H, W, TR, TC, rstep, cstep, Cs=4, M=2, index=None, flip=None, C=None, H0=None, W0=None, off=None,
          expect=None, seed=0):
    H0 = (H - 1) * rstep + TR if H0 is None else H0                 # exact fit: the last start is n_in - taps
    W0 = (W - 1) * cstep + TC if W0 is None else W0
    if kind == "f32":
        Cs = 4
        index = list(range(M))
    elif index is None:
        index = {1: [0, 0], 2: [1, 0, 1], 3: [2, 0, 2, 1]}[M]       # repeated, out of order, includes M - 1
    flip = [(k + seed) % 2 for k in range(len(index))] if flip is None else flip      # mixed
    C = list(range(1, Cs + 1)) if C is None else C
    nbytes = M * H0 * W0 * (Cs if kind == "u8" else 16)
    assert nbytes < SOURCE_LIMIT, (name, nbytes)
    return dict(name=name, kind=kind, H=H, W=W, TR=TR, TC=TC, rstep=rstep, cstep=cstep, Cs=Cs, M=M, index=index,
                flip=[int(bool(f)) for f in flip], C=C, H0=H0, W0=W0, off=off, expect=expect, seed=seed, nbytes=nbytes)


TAIL_H, TAIL_W = (7, 8, 9, 17), (1, 63, 64, 65, 255, 256, 257, 513)
TAIL_TR, TAIL_TC, TAIL_RSTEP = (1, 3, 5), (1, 4), (0, 1, 3)


def _tail_cases(kind):
    """Every (H, W) pair of the tail grid once; TR, TC, the row step, the column step, Cs, C and M rotate so that each value meets
    each H and each W class.  Wide outputs keep a column step of 1 (and f32 sources fewer rows) to stay below SOURCE_LIMIT."""
    out = []
    for n, (H, W) in enumerate(itertools.product(TAIL_H, TAIL_W)):
        TR, TC, rstep = TAIL_TR[n % 3], TAIL_TC[(n // 3) % 2], TAIL_RSTEP[(n // 2) % 3]
        cstep = (0, 1, 2, 3)[(n + n // 8) % 4]
        Cs = 3 + n % 2 if kind == "u8" else 4
        M = 2 + (n // 4) % 2

        def nbytes():
            H0 = TR + 2 if rstep == 0 else (H - 1) * rstep + TR
            W0 = TC + 3 if cstep == 0 else (W - 1) * cstep + TC
            return M * H0 * W0 * (Cs if kind == "u8" else 16), H0, W0
        if nbytes()[0] >= SOURCE_LIMIT:
            M = 2 if kind == "u8" else 1
        if nbytes()[0] >= SOURCE_LIMIT:
            rstep = 1
        if nbytes()[0] >= SOURCE_LIMIT:
            cstep = 1
        _, H0, W0 = nbytes()          # step 0: every output reads the same taps; two rows / three columns more are never read
        out.append(_case(f"tail-{kind}-H{H}-W{W}-TR{TR}-TC{TC}-rs{rstep}-cs{cstep}-Cs{Cs}-M{M}", kind, H, W, TR, TC, rstep, cstep,
                         Cs=Cs, M=M, C=[1 + (n % Cs)], H0=H0, W0=W0, seed=n))
    return out


def _rq_cases():
    """W = 256, column step 4, W0 = 1100: the tap count moves the weight tile through the LDS budget and rq through its classes.
    The row band of the first block is 19 source rows (9 output rows, step 2, 5 taps): never a multiple of rq > 1."""
    out = []
    for Cs, plan in ((4, ((8, 8), (32, 7), (48, 3), (56, 1), (64, "refused"))),
                     (3, ((8, 8), (32, 8), (48, 5), (56, 2), (60, 1), (64, "refused")))):
        for TC, expect in plan:
            out.append(_case(f"rq-u8-Cs{Cs}-TC{TC}-{expect}", "u8", 9, 256, 5, TC, 2, 4, Cs=Cs, M=1, index=[0, 0], flip=[0, 1],
                             C=[Cs], H0=24, W0=1100, expect=expect, seed=TC + Cs))
    out.append(_case("rq-f32-TC4-step1-8", "f32", 5, 256, 3, 4, 2, 1, M=2, flip=[1, 0], C=[3], H0=11, W0=300, expect=8, seed=1))
    for TC, expect in ((8, 3), (32, 1), (48, "refused")):
        out.append(_case(f"rq-f32-TC{TC}-{expect}", "f32", 5, 256, 3, TC, 2, 4, M=1, flip=[1], C=[3], H0=11, W0=1100, expect=expect, seed=TC))
    return out


def _other_cases():
    # one pixel: the source is Cs bytes long; as a fresh allocation (the end of the buffer inside the first 16-byte piece) and as an
    # offset view behind 255s (the piece starts before the buffer as well)
    out = [_case(f"single-Cs{Cs}" + (f"-off{off}" if off else ""), "u8", 1, 1, 1, 1, 0, 0, Cs=Cs, M=1, index=[0], flip=[Cs == 4],
                 off=off, seed=Cs) for Cs, offs in ((3, (None, 5)), (4, (None, 4))) for off in offs]
    # alignment: odd W0, every source row staged (7 output rows, 3 taps, step 1 over 9 rows), the source an offset view
    for Cs, offs in ((3, (1, 5, 15)), (4, (4, 12))):
        for off in offs:
            out.append(_case(f"align-Cs{Cs}-off{off}", "u8", 7, 34, 3, 4, 1, 1, Cs=Cs, M=2, index=[1, 0, 1, 1], flip=[0, 1, 1, 0],
                             H0=9, W0=37, off=off, seed=off))
    # degenerate bands
    out.append(_case("degen-colstep0-TC=W0", "u8", 9, 70, 3, 12, 1, 0, Cs=3, M=2, W0=12, seed=1))
    out.append(_case("degen-TR=H0", "u8", 9, 65, 6, 4, 0, 2, Cs=4, M=3, H0=6, seed=2))
    out.append(_case("degen-span-clamped-by-W0", "u8", 9, 64, 3, 4, 1, 3, Cs=3, M=2, W0=100, seed=3))
    out.append(_case("degen-last-starts-at-the-end", "u8", 17, 257, 5, 4, 3, 2, Cs=3, M=2, C=[3], seed=4))
    out.append(_case("degen-f32-colstep0-TR=H0", "f32", 9, 70, 6, 12, 0, 0, M=2, H0=6, W0=12, seed=5))
    # flip over a ragged second tile
    for Cs in (3, 4):
        out.append(_case(f"flip-W257-Cs{Cs}", "u8", 9, 257, 3, 4, 1, 1, Cs=Cs, M=2, index=[1, 1, 0, 0], flip=[0, 1, 1, 0], C=[Cs], seed=Cs))
    out.append(_case("flip-f32-W257", "f32", 9, 257, 3, 4, 1, 1, M=2, flip=[0, 1], C=[4], seed=6))
    return out


CASES = {c["name"]: c for c in _tail_cases("u8") + _tail_cases("f32") + _rq_cases() + _other_cases()}


def names(kind, prefix=""):
    return [n for n, c in CASES.items() if c["kind"] == kind and n.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def build(name):
    """-> (case, src, rows, cols): the source (u8: (M,H0,W0,Cs) uint8; f32: (M,H0,W0,4) float32 values k/256) and the two integer
    tables of a case.  Computed once and shared; callers must not write to it."""
    c = CASES[name]
    rng = np.random.default_rng(1000 + c["seed"] + 7 * len(name))
    shape = (c["M"], c["H0"], c["W0"], c["Cs"])
    if c["kind"] == "u8":
        src = rng.integers(0, 256, shape, dtype=np.uint8)
        if c["H0"] * c["W0"] >= 4:                                 # saturated corners (not where they would be the whole source)
            src[0, :1, :2] = 255
            src[-1, -1:, -2:] = 0
    else:
        src = (rng.integers(0, 257, shape).astype(np.float64) / 256.0).astype(F32)
        if c["H0"] * c["W0"] >= 4:
            src[0, :1, :2] = 1.0
    rows = make_table(rng, c["H0"], c["H"], c["TR"], c["rstep"])
    cols = make_table(rng, c["W0"], c["W"], c["TC"], c["cstep"])
    for a in (src, *rows[:2], *cols[:2]):
        a.setflags(write=False)
    return c, src, rows, cols


def plan_of(name):
    c, _, rows, cols = build(name)
    return resample_plan(c["kind"], c["H0"], c["W0"], c["H"], c["W"], c["TR"], c["TC"], cols[2], c["Cs"], rows[1], cols[1])


def resample_int(name):
    """Exact per-source result as integers: value * 256 * 255 (u8) or value * 65536 (f32 sources k/256), (M, H, W, Cs)."""
    c, src, rows, cols = build(name)
    x = src.astype(np.int64) if c["kind"] == "u8" else np.rint(src.astype(np.float64) * 256.0).astype(np.int64)
    return band_int(band_int(x, cols, 2), rows, 1)


def resample_f32_statement(name):
    """The kernels' float32 arithmetic before the division: horizontal pass (taps ascending), then vertical (rows ascending)."""
    c, src, rows, cols = build(name)
    return band_f32(band_f32(src.astype(F32), cols, 2), rows, 1)


@functools.lru_cache(maxsize=None)
def resample_values(name):
    """(M, H, W, Cs) float32: what the kernel holds for every source before channel selection, flip and store."""
    c = CASES[name]
    acc = resample_int(name)
    if c["kind"] == "u8":
        v = (acc.astype(F32) / F32(256)) / F32(255)                # acc / 256 is exact; ONE rounding, the division by 255.0f
    else:
        v = acc.astype(F32) / F32(65536)                           # exact
    assert v.dtype == F32
    v.setflags(write=False)
    return v


def resample_expect(name, C, bf16=False):
    """(N, H, W, 8) float32: channels < C of source index[n], reversed along W where flip[n], channels C..7 zero; bf16: the same
    rounded to nearest-even."""
    c = CASES[name]
    v = resample_values(name)
    out = np.zeros((len(c["index"]), c["H"], c["W"], CPAD), F32)
    for n, (i, f) in enumerate(zip(c["index"], c["flip"])):
        out[n, ..., :C] = (v[i][:, ::-1] if f else v[i])[..., :C]
    return bf16_rne(out) if bf16 else out


# ---------------------------------------------------------------------------------------------------------- warp
WARP_S = (1, 15, 16, 17, 63, 64, 65, 80)
WARP_TABLES = ("W0=S,TC=1", "W0=2S,TC=2", "W0=3S+1,TC=4")


def warp_table(S, which):
    """The squaring band table (W0 -> S columns): identity; pairs averaged (1/2, 1/2); four taps at step 3 with zero weights
    and a last start of W0 - TC."""
    if which == WARP_TABLES[0]:
        return S, (np.full((S, 1), 16, np.int64), np.arange(S, dtype=np.int32), 1 if S > 1 else 0)
    if which == WARP_TABLES[1]:
        return 2 * S, (np.full((S, 2), 8, np.int64), (2 * np.arange(S)).astype(np.int32), 2 if S > 1 else 0)
    W0 = 3 * S + 1
    tab = make_table(np.random.default_rng(40 + S), W0, S, 4, 3)
    assert tab[1][-1] == W0 - 4
    return W0, tab


def _m(a, b, c, d, e, f):
    return np.array([[a, b, c], [d, e, f]], np.float64)


def _shift(sx, sy):
    return _m(1, 0, sx, 0, 1, sy)


IDENT = _m(1, 0, 0, 0, 1, 0)


def warp_groups(S):
    """{group: [(name, (2,2,3) float64 [fill, sample])]}: the maps of one launch each.  Groups keep maps of one window class
    together (data.warp_window takes the largest extent over a launch)."""
    T, k, S2 = S // 3, S // 4, float(2 * S)
    same = lambda name, m: (name, np.stack([m, m]))
    filled = lambda name, m: (name, np.stack([IDENT, m]))
    unit = [same("identity", IDENT), same("flip-x", _m(-1, 0, S, 0, 1, 0)), same("flip-y", _m(1, 0, 0, 0, -1, S)),
            same("flip-xy", _m(-1, 0, S, 0, -1, S))]
    for s in (-0.5, 0.5, -1.0, 1.0):
        unit += [same(f"shift-x{s:+}", _shift(s, 0)), same(f"shift-y{s:+}", _shift(0, s))]
    unit += [same("shift-xy-half", _shift(-0.5, 0.5)), same("flip-x-shift-half", _m(-1, 0, S + 0.5, 0, 1, -0.5))]
    unit += [same(f"translate{tx:+}{ty:+}", _shift(tx, ty)) for tx, ty in ((T, 0), (-T, 0), (0, T), (0, -T), (T, -T), (-T, T))]
    unit += [("fill-all-outside", np.stack([_shift(S2, 0), IDENT])), ("fill-all-outside-y", np.stack([_shift(0, -S2), _m(-1, 0, S, 0, 1, 0)])),
             filled("sample+2S", _shift(S2, S2)), filled("sample-2S", _shift(-S2, -S2)), filled("sample+2S-x-only", _shift(S2, 0))]
    half = [filled("half", _m(0.5, 0, k + 0.25, 0, 0.5, k + 0.25)),
            filled("half-flip-x", _m(-0.5, 0, S - k - 0.25, 0, 0.5, 0.25)),
            filled("half-x-only", _m(0.5, 0, 0.25, 0, 1, 0))]
    double = [filled("double", _m(2, 0, -(S // 2), 0, 2, -(S // 2) - 0.5)), filled("double-x", _m(2, 0, 0, 0, 1, 0)),
              filled("double-flip", _m(-2, 0, 2 * S - 0.5, 0, 2, -0.5))]
    swap = [filled("swap", _m(0, 1, 0, 1, 0, 0)), same("swap-flip", _m(0, -1, S, 1, 0, 0)), filled("swap-half-shift", _m(0, 1, 0.5, -1, 0, S))]
    return {"unit": unit, "half": half, "double": double, "swap": swap}


@functools.lru_cache(maxsize=None)
def warp_source(S, Cs, which):
    """(2, S, W0, Cs) uint8 and the integer table; shared, read-only."""
    W0, tab = warp_table(S, which)
    src = np.random.default_rng(S * 100 + Cs * 10 + W0).integers(0, 256, (2, S, W0, Cs), dtype=np.uint8)
    src[0, 0, 0] = 255
    src[1, -1, -1] = 0
    assert src.nbytes < SOURCE_LIMIT
    src.setflags(write=False)
    return src, tab


def squared_int(img, tab):
    """(S, S, 3) int64: the horizontal band sums of one (S, W0, Cs) image x 16 (exact)."""
    return band_int(np.asarray(img)[..., :3], tab, 1)


def squared_f32(img, tab):
    """A as the kernel forms it in LDS: the exact horizontal sum, then ONE rounding in the division by 255.0f."""
    return (squared_int(img, tab).astype(F32) / F32(16)) / F32(255)


def warp_points(mats, S):
    """inside (S,S) bool, u, v (float64): fill decision and neighbour coordinates, each (m0*px + m1*py) + m2 (- 0.5)."""
    py, px = np.meshgrid(np.arange(S) + 0.5, np.arange(S) + 0.5, indexing="ij")
    f, s = np.asarray(mats, np.float64)
    fx, fy = (f[0, 0] * px + f[0, 1] * py) + f[0, 2], (f[1, 0] * px + f[1, 1] * py) + f[1, 2]
    u, v = ((s[0, 0] * px + s[0, 1] * py) + s[0, 2]) - 0.5, ((s[1, 0] * px + s[1, 1] * py) + s[1, 2]) - 0.5
    return (fx >= 0.0) & (fx <= S) & (fy >= 0.0) & (fy <= S), u, v


def warp_neighbours(mats, S):
    """inside, (ya, yb, xa, xb) clamped neighbour indices, (w00, w01, w10, w11) float32 weights."""
    inside, u, v = warp_points(mats, S)
    fu, fv = np.floor(u), np.floor(v)
    bx, by = u - fu, v - fv
    ix, iy = np.clip(fu, -1, S).astype(np.int64), np.clip(fv, -1, S).astype(np.int64)
    idx = (np.clip(iy, 0, S - 1), np.clip(iy + 1, 0, S - 1), np.clip(ix, 0, S - 1), np.clip(ix + 1, 0, S - 1))
    w = (((1.0 - by) * (1.0 - bx)).astype(F32), ((1.0 - by) * bx).astype(F32), (by * (1.0 - bx)).astype(F32), (by * bx).astype(F32))
    return inside, idx, w


def warp_expect(A32, mats):
    """(S, S, 4) float32: the kernel's float32 statement for one sample.  A32 (S,S,3) float32 from squared_f32."""
    S = A32.shape[0]
    inside, (ya, yb, xa, xb), (w00, w01, w10, w11) = warp_neighbours(mats, S)
    e = (Ellipsis, None)
    o = w00[e] * A32[ya, xa]
    o = w01[e] * A32[ya, xb] + o
    o = w10[e] * A32[yb, xa] + o
    o = w11[e] * A32[yb, xb] + o
    assert o.dtype == F32
    out = np.zeros((S, S, 4), F32)
    out[..., :3] = np.where(inside[e], o, F32(0))
    return out


def warp_plan(mats, S, window):
    """The launch of sgg_warp_affine_u8 restated for (N,2,2,3) matrices: the LDS window (clamped to S, refused above 64 KB), and
    per sample and tile the origin taken from the four tile corners.  covered: every neighbour of every pixel inside the image
    lies in its tile's window, so clamping to the window changes nothing and warp_expect is what the kernel must give."""
    wh, ww = min(int(window[0]), S), min(int(window[1]), S)
    p = dict(wh=wh, ww=ww, lds=16 * wh * ww, refused=16 * wh * ww > WP_LDS, rows_clamped=window[0] > S, cols_clamped=window[1] > S)
    if p["refused"]:
        return p
    covered, origins, outside_tiles, tiles = True, set(), 0, 0
    for m in np.asarray(mats, np.float64):
        inside, (ya, yb, xa, xb), _ = warp_neighbours(m, S)
        s = m[1]
        for y0, x0 in itertools.product(range(0, S, WP_TH), range(0, S, WP_TW)):
            cx = np.array([x0 + 0.5, x0 + WP_TW - 0.5, x0 + 0.5, x0 + WP_TW - 0.5])
            cy = np.array([y0 + 0.5, y0 + 0.5, y0 + WP_TH - 0.5, y0 + WP_TH - 0.5])
            umin = (((s[0, 0] * cx + s[0, 1] * cy) + s[0, 2]) - 0.5).min()
            vmin = (((s[1, 0] * cx + s[1, 1] * cy) + s[1, 2]) - 0.5).min()
            ox, oy = int(np.clip(np.floor(umin), 0, S - 1)), int(np.clip(np.floor(vmin), 0, S - 1))
            origins.add((ox, oy))
            t = (slice(y0, y0 + WP_TH), slice(x0, x0 + WP_TW))
            ins = inside[t]
            tiles += 1
            outside_tiles += int(not ins.any())
            for a, o, n in ((xa, ox, ww), (xb, ox, ww), (ya, oy, wh), (yb, oy, wh)):
                r = a[t][ins] - o
                covered &= bool(((r >= 0) & (r < n)).all())
    p.update(covered=covered, origins=origins, outside_tiles=outside_tiles, tiles=tiles)
    return p
