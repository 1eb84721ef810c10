"""Float64 statement of the data-parallel train step, test infrastructure only: what ONE rank computes -- the composed
oracle (tests/composed_oracle.py, tests/featmatch_oracle.py) on the rank's rows of the batch, its draws taken at the rank's sample
offset ``rank * n`` -- and what every rank holds after the exchange: ``exchanged``, the sum of the ranks' gradients as the buffers
hold it before a spectral discriminator's transform, and ``network_after_exchange``, composed_oracle.network_update ONCE on that sum
with ``grad_scale = 1 / world``.  tests/test_dp_oracle_cpu.py holds the statement to the concatenated-batch oracle and shows that
the errors a data-parallel step can make move it beyond the bounds of tests/test_gpu_dp_options.py."""
import numpy as np

from tests import composed_oracle as CO
from tests import diffaug_oracle as DA
from tests import featmatch_oracle as FM
from tests import spectral_oracle as S

F64 = np.float64
H = W = 128
C8 = 64                                     # the channels of d1..d3 at ngf 8
# the bounds of the single-process files (tests/test_gpu_composed.py), unchanged
LOSS_TOL, GRAD_TOL, UPDATE_TOL, U32 = 2e-5, 2e-4, 2e-6, 2.0 ** -24


# ---- the fixed cases of tests/test_gpu_dp_options.py (global batch 2, one sample per rank; their first steps are the first steps of
# tests/test_gpu_composed.py's and tests/test_gpu_featmatch.py's cases; ambiguity caps: tests/test_dp_oracle_cpu.py) ----------------
WORLD = 2


def reference_case(steps=3, N=2):
    """({"Gab", "Da"}, [(real, seg, mask) per step]) -- the U-Net reference step, every option on."""
    rng = np.random.default_rng(CO.REFERENCE_CASE_SEED)
    return CO.case_params(rng, False), [CO.case_inputs(rng, N) for _ in range(steps)]


def cycle_case(steps=2, N=2):
    """({"Gab", "Gba", "Da", "Db"}, [((real_A, seg_A, mask_A), (real_B, seg_B, mask_B)) per step])."""
    rng = np.random.default_rng(CO.CYCLE_CASE_SEED)
    return CO.case_params(rng, True), [(CO.case_inputs(rng, N), CO.case_inputs(rng, N)) for _ in range(steps)]


def featmatch_case(N=2):
    """featmatch_oracle.case("composed"): ({"Gab", "Da"}, its u, (real, seg, mask))."""
    _, P, U, inputs = FM.case("composed", N)
    return P, U, inputs


# ---- a rank's share of a step -----------------------------------------------------------------------------------------------------
def rows_of(arrays, rank, n):
    return tuple(np.asarray(a)[rank * n:(rank + 1) * n] for a in arrays)


def reference_rows(t, n, rank, seed=CO.SEED, policy=CO.POLICY):
    """sggan.diffaug_params of a reference step on rank ``rank`` holding n samples: [reals; fakes] of the global samples rank * n .."""
    return np.concatenate([DA.param_rows(t, seed, rank * n, n, role, H, W, policy) for role in (0, 1)])


def cycle_rows(ta, tb, n, rank, seed=CO.SEED, policy=CO.POLICY):
    """... of a cycle step: [D_B reals; D_B fakes; D_A fakes; D_A reals]."""
    off = rank * n
    return np.concatenate([DA.param_rows(tb, seed, off, n, 2, H, W, policy), DA.param_rows(tb, seed, off, n, 3, H, W, policy),
                           DA.param_rows(ta, seed, off, n, 1, H, W, policy), DA.param_rows(ta, seed, off, n, 0, H, W, policy)])


def generator_masks(t, seed, application, n, rank):
    return CO.generator_masks(t, seed, application, n, H, W, C8, sample_offset=rank * n)


def cycle_masks(t_ab, t_ba, n, rank, seed=CO.SEED):
    return {("Gab", a): generator_masks(t_ab, seed, a, n, rank) for a in (0, 1)} | \
           {("Gba", a): generator_masks(t_ba, seed + 2, a, n, rank) for a in (0, 1)}


def normal(r):
    """One layout for the results of composed_oracle.reference_step / cycle_step and featmatch_oracle.reference_step:
    {"losses": (generator, discriminator), "grads": {net: {name: array}}, "scaled": {net: {layer: dL / d(W / sigma)} or None},
    "U" / "V" / "sigma": {net: ...}} with the networks named as tests/test_gpu_composed._nets names them."""
    if "grads" in r:
        return {"losses": (r["g_loss"], r["d_loss"]), "grads": r["grads"], "scaled": r["scaled"], "U": {"Da": r["Ua"], "Db": r["Ub"]},
                "V": {"Da": r["Va"], "Db": r["Vb"]}, "sigma": {"Da": r["sigma_a"], "Db": r["sigma_b"]},
                "images": {k: r[k] for k in ("fake_A", "fake_B", "cyc_A", "cyc_B")}}
    return {"losses": (r["gen_loss"], r["disc_loss"]), "grads": {"Gab": r["gG"], "Da": r["gD"]}, "scaled": {"Da": r["gD_scaled"]},
            "U": {"Da": r["U"]}, "V": {"Da": r["V"]}, "sigma": {"Da": r["sigma"]}, "features": r.get("features")}


def reference_rank_step(P, U, inputs, rank, n, tG, tD, *, seed=CO.SEED, draws_of=None, options=True):
    """Rank ``rank``'s reference step with every option on (options=False: none) from the parameters P = {"Gab", "Da"} and D's u.
    ``inputs``: the GLOBAL batch (real, seg, mask); the rank takes its rows.  draws_of: the rank whose offset keys the draws (the
    planted error "rank 1 draws with offset 0"); None: its own."""
    real, seg, mask = rows_of(inputs, rank, n)
    k = rank if draws_of is None else draws_of
    if not options:
        return normal(CO.reference_step(P["Gab"], P["Da"], U, real, seg, mask))
    return normal(CO.reference_step(P["Gab"], P["Da"], U, real, seg, mask, masks=generator_masks(tG, seed, 0, n, k),
                                    rows=reference_rows(tD, n, k, seed), ssim_lambda=CO.SSIM_LAMBDA))


def cycle_rank_step(P, Ua, Ub, inputs_A, inputs_B, rank, n, t, *, seed=CO.SEED, signs=None, draws_of=None):
    """Rank ``rank``'s cycle step with every option on; t = {"Gab", "Gba", "Da", "Db"}: the counters before the step."""
    (rA, sA, mA), (rB, sB, mB) = rows_of(inputs_A, rank, n), rows_of(inputs_B, rank, n)
    k = rank if draws_of is None else draws_of
    return normal(CO.cycle_step(P["Gab"], P["Gba"], P["Da"], P["Db"], Ua, Ub, rA, rB, sA, sB, mA, mB,
                                masks=cycle_masks(t["Gab"], t["Gba"], n, k, seed), rows=cycle_rows(t["Da"], t["Db"], n, k, seed),
                                ssim_lambda=CO.SSIM_LAMBDA, signs=signs))


def featmatch_rank_step(P, U, inputs, rank, n, **kw):
    """Rank ``rank``'s step of featmatch_oracle's "composed" case (ResNet generator, spectral D, the SSIM term, fm_lambda)."""
    return normal(FM.case_step("composed", P, U, rows_of(inputs, rank, n), **kw))


# ---- after the exchange -------------------------------------------------------------------------------------------------------------
def exchanged(ranks, net):
    """What network ``net``'s gradient buffer holds on EVERY rank once the all-reduce has completed: the sum over ``ranks`` (their
    ``normal`` results) -- for a spectral discriminator the gradients with respect to W / sigma under ``<layer>_w``, as the kernels
    leave them before spectral_grad."""
    out = {k: sum(np.asarray(r["grads"][net][k], F64) for r in ranks) for k in ranks[0]["grads"][net]}
    if ranks[0]["scaled"].get(net) is not None:
        for layer in S.LAYERS:
            out[layer + "_w"] = sum(np.asarray(r["scaled"][net][layer], F64) for r in ranks)
    return out


def mean_losses(ranks):
    return tuple(float(np.mean([r["losses"][i] for r in ranks])) for i in (0, 1))


def network_after_exchange(theta, m, v, t, ema, ranks, net, *, lr, max_norm, sched, ema_decay=None, beta1=0.5, grad_scale=None,
                           spectral=None, buffer=None):
    """The state of ``net`` after the step on every rank, from its state before (theta, m, v, ema: {name: array}; t: Adam's
    counter) and the ranks' oracle results: the summed buffer, then composed_oracle.network_update ONCE with grad_scale = 1 / world
    -- the spectral transform (W = theta; u, v, sigma as rank 0 states them: every rank holds the same), the norm of the
    transformed sum times 1 / world, the clip, the scheduled rate, Adam, the average.  grad_scale / spectral override the two for
    the planted errors.  ``buffer``: an exchanged buffer to go on from in place of the oracle's sum (a spectral discriminator's is
    taken as already transformed unless ``spectral`` is given) -- the device's own, which the
    GPU tests hold to that sum separately: Adam divides by |g|, so a parameter whose gradient lies within the kernels' rounding of
    zero moves by up to the rate whichever sign the rounding leaves, and theta is comparable at 2e-6 only from the buffer the
    update really read (tests/test_gpu_composed.py's update-chain test does the same).  Returns composed_oracle.network_update's
    tuple; info["buffer"] is the buffer used."""
    buf = exchanged(ranks, net) if buffer is None else buffer
    if spectral is None and buffer is None and ranks[0]["scaled"].get(net) is not None:
        spectral = (theta, ranks[0]["U"][net], ranks[0]["V"][net], ranks[0]["sigma"][net])
    scale = 1.0 / len(ranks) if grad_scale is None else grad_scale
    th, m1, v1, it, e1, info = CO.network_update(theta, buf, m, v, t, ema, lr=lr, beta1=beta1, grad_scale=scale, max_norm=max_norm,
                                                 sched=sched, ema_decay=ema_decay, spectral=spectral)
    return th, m1, v1, it, e1, dict(info, buffer=buf)


# ---- comparisons at the GPU tests' bounds -----------------------------------------------------------------------------------------
def worst(got, exp):
    """{name: (relative L2, worst entry over largest)} over the tensors of ``exp`` that are not identically zero."""
    out = {}
    for k, e in exp.items():
        e = np.asarray(e, F64)
        if np.abs(e).max() < 1e-9:
            continue
        d = np.asarray(got[k], F64) - e
        out[k] = (float(np.sqrt((d ** 2).sum()) / np.sqrt((e ** 2).sum())), float(np.abs(d).max() / np.abs(e).max()))
    return out


def grads_beyond(got, exp, tol=GRAD_TOL):
    return {k: v for k, v in worst(got, exp).items() if not (v[0] < tol and v[1] < tol)}


def update_beyond(got, exp, k=1):
    """The entries of two network_after_exchange results (or a device state in the same layout) further apart than the GPU tests
    allow: theta, m, v at 2e-6, the counter exactly, norm and clip of the guard's record at the gradients' 2e-4, the average at
    3 k 2^-24 of its largest entry + 2e-6."""
    flat = lambda d: np.concatenate([np.asarray(x, F64).reshape(-1) for x in d.values()])
    bad = {}
    for i, what in enumerate(("theta", "m", "v")):
        err = float(np.abs(flat(got[i]) - flat(exp[i])).max())
        if not err < UPDATE_TOL:
            bad[what] = err
    if got[3] != exp[3]:
        bad["t"] = (got[3], exp[3])
    if exp[4] is not None:
        e = flat(exp[4])
        err = float(np.abs(flat(got[4]) - e).max())
        if not err <= 3 * k * U32 * float(np.abs(e).max()) + UPDATE_TOL:
            bad["ema"] = err
    for what in ("norm", "clip"):
        a, b = got[5][what], exp[5][what]
        if not abs(a - b) <= GRAD_TOL * abs(b):
            bad[what] = (a, b)
    if got[5]["skip"] != exp[5]["skip"]:
        bad["skip"] = (got[5]["skip"], exp[5]["skip"])
    return bad
