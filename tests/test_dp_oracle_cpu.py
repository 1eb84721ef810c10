"""What tests/test_gpu_dp_options.py rests on, checked without a GPU (tests/dp_oracle.py):

a. the partition property -- in float64 the composed oracle on the concatenated batch is the mean over ranks of the oracle on each
   rank's rows, its draws taken at sample offset rank * n: losses and every gradient tensor at 1e-11 (only the order of the sums
   over the batch differs), u after the step identical;
b. the expected-state builder, dp_oracle.network_after_exchange, is composed_oracle.network_update on the concatenated batch;
c. each error a data-parallel step can make moves the result beyond the GPU tests' bounds;
d. the GPU cases' inputs stay under the ambiguity cap of tests/test_composed_cpu.py and tests/test_featmatch_cpu.py.

Global batch 2, one sample per rank, 128 x 128 (the smallest size the U-Net and the 1 x 1 head accept); every oracle step is
evaluated once per module."""
import numpy as np
import pytest

from tests import composed_oracle as CO
from tests import dp_oracle as DP
from tests import featmatch_oracle as FM
from tests import spectral_oracle as S

H = W = DP.H
PARTITION = 1e-11
CAP = 5e-3                      # of the sign() arguments within 1e-4 of zero (featmatch_oracle.CAP)
SCHED = (1, 1, 4)               # tests/test_gpu_composed.py's
EMA_DECAY = 0.999


def _err(got, exp):
    return float(np.abs(np.asarray(got, np.float64) - exp).max() / max(np.abs(exp).max(), 1e-300))


def _partition(whole, ranks, what):
    """``whole``: the concatenated batch's result, ``ranks``: the ranks' (dp_oracle.normal layout)."""
    for a, b in zip(whole["losses"], DP.mean_losses(ranks)):
        assert abs(a - b) <= PARTITION * abs(a), (what, a, b)
    world = len(ranks)
    worst = (0.0, None)
    for net, grads in whole["grads"].items():
        mean = {k: v / world for k, v in DP.exchanged(ranks, net).items()}
        exp = dict(grads)
        if whole["scaled"].get(net) is not None:        # the buffer holds dL / d(W / sigma) under the kernels' names
            exp.update({layer + "_w": whole["scaled"][net][layer] for layer in S.LAYERS})
        assert set(mean) == set(exp)
        for k, e in exp.items():
            if np.abs(e).max() < 1e-9:                  # (a bias in front of an unmasked instance norm: rounding noise on both sides)
                assert np.abs(mean[k]).max() < 1e-9, (what, net, k)
                continue
            worst = max(worst, (_err(mean[k], e), (net, k)))
        # ... and the gradient with respect to W itself, which the transform of the summed buffer has to reproduce
        for k, e in grads.items():
            if np.abs(e).max() >= 1e-9:
                worst = max(worst, (_err(sum(r["grads"][net][k] for r in ranks) / world, e), (net, k, "W")))
    print(f"{what}: worst tensor {worst[1]} at {worst[0]:.2e} of its largest entry")
    assert worst[0] <= PARTITION, (what, worst)
    for net, U1 in whole["U"].items():                  # u after the step: a function of the kernels and u alone
        if U1 is not None:
            assert all(np.array_equal(U1[n], r["U"][net][n]) for r in ranks for n in S.LAYERS), (what, net)


# ---- the cases, evaluated once ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference():
    P, inputs = DP.reference_case(steps=1)
    U = S.init_u(S.discriminator_param_shapes(df_dim=8), np.random.default_rng(5))
    whole = DP.normal(CO.reference_step(P["Gab"], P["Da"], U, *inputs[0], masks=CO.generator_masks(0, CO.SEED, 0, 2, H, W, DP.C8),
                                        rows=CO.reference_rows(0, 2, H, W), ssim_lambda=CO.SSIM_LAMBDA))
    ranks = [DP.reference_rank_step(P, U, inputs[0], r, 1, 0, 0) for r in range(2)]
    return {"P": P, "U": U, "inputs": inputs[0], "whole": whole, "ranks": ranks}


@pytest.fixture(scope="module")
def cycle():
    P, inputs = DP.cycle_case(steps=1)
    shapes, rng = S.discriminator_param_shapes(df_dim=8), np.random.default_rng(6)
    Ua, Ub = S.init_u(shapes, rng), S.init_u(shapes, rng)
    (rA, sA, mA), (rB, sB, mB) = inputs[0]
    raw = CO.cycle_step(P["Gab"], P["Gba"], P["Da"], P["Db"], Ua, Ub, rA, rB, sA, sB, mA, mB, masks=CO.cycle_masks(0, 0, 2, H, W, DP.C8),
                        rows=CO.cycle_rows(0, 0, 2, H, W), ssim_lambda=CO.SSIM_LAMBDA)
    t = dict.fromkeys(("Gab", "Gba", "Da", "Db"), 0)
    ranks = [DP.cycle_rank_step(P, Ua, Ub, *inputs[0], r, 1, t) for r in range(2)]
    return {"inputs": inputs[0], "raw": raw, "whole": DP.normal(raw), "ranks": ranks}


@pytest.fixture(scope="module")
def featmatch():
    P, U, inputs = DP.featmatch_case()
    whole = DP.normal(FM.case_step("composed", P, U, inputs))
    return {"whole": whole, "ranks": [DP.featmatch_rank_step(P, U, inputs, r, 1) for r in range(2)]}


# ---- a. the partition property -----------------------------------------------------------------------------------------------------
def test_reference_step_on_the_concatenated_batch_is_the_mean_of_the_ranks(reference):
    _partition(reference["whole"], reference["ranks"], "reference step, every option on")
    # the two ranks' draws are rows [r, r + 1) of the single-device run's, and differ from each other
    rows = CO.reference_rows(0, 2, H, W).view(np.uint32)
    for r in range(2):
        assert np.array_equal(DP.reference_rows(0, 1, r).view(np.uint32), rows[[r, 2 + r]])
        for whole, mine in zip(CO.generator_masks(0, CO.SEED, 0, 2, H, W, DP.C8), DP.generator_masks(0, CO.SEED, 0, 1, r)):
            assert np.array_equal(whole[r:r + 1], mine)
    assert not np.array_equal(rows[0], rows[1])


def test_cycle_step_on_the_concatenated_batch_is_the_mean_of_the_ranks(cycle):
    _partition(cycle["whole"], cycle["ranks"], "cycle step, every option on")
    rows = CO.cycle_rows(0, 0, 2, H, W).view(np.uint32)
    for r in range(2):
        assert np.array_equal(DP.cycle_rows(0, 0, 1, r).view(np.uint32), rows[[r, 2 + r, 4 + r, 6 + r]])


def test_feature_matching_step_on_the_concatenated_batch_is_the_mean_of_the_ranks(featmatch):
    _partition(featmatch["whole"], featmatch["ranks"], "reference step with the feature-matching term")


# ---- b. the expected-state builder ---------------------------------------------------------------------------------------------------
LR = {"Gab": 1e-3, "Da": 1e-3}              # sggan.LR, the reference step's


def _zeros(P):
    return {k: np.zeros_like(v) for k, v in P.items()}


def _probe_norms(case):
    return {net: DP.network_after_exchange(case["P"][net], _zeros(case["P"][net]), _zeros(case["P"][net]), 0, None, case["ranks"], net,
                                           lr=LR[net], max_norm=0.0, sched=SCHED)[5]["norm"] for net in ("Gab", "Da")}


@pytest.fixture(scope="module")
def stepped(reference):
    """The reference case one correct step on: {net: (theta, m, v, t, ema)} at t = 1 -- slots non-zero, the average off the
    parameters -- and the clip bound the GPU tests use, a quarter of the smallest norm."""
    norms = _probe_norms(reference)
    bound = 0.25 * min(norms.values())
    state = {}
    for net in ("Gab", "Da"):
        P = reference["P"][net]
        ema = dict(P) if net == "Gab" else None
        state[net] = DP.network_after_exchange(P, _zeros(P), _zeros(P), 0, ema, reference["ranks"], net, lr=LR[net], max_norm=bound,
                                               sched=SCHED, ema_decay=EMA_DECAY if net == "Gab" else None)
        assert state[net][3] == 1 and state[net][5]["clip"] < 1.0
    return state, bound


def _second(reference, stepped, net, ranks=None, **over):
    """The second step of ``net`` from ``stepped`` (the same gradients again: only the update chain is looked at)."""
    state, bound = stepped
    th, m, v, t, ema, _ = state[net]
    kw = dict(lr=LR[net], max_norm=bound, sched=SCHED, ema_decay=EMA_DECAY if net == "Gab" else None)
    kw.update({k: over.pop(k) for k in list(over) if k in ("max_norm", "grad_scale", "spectral")})
    th, m, v, t, ema = over.get("theta", th), over.get("m", m), over.get("v", v), over.get("t", t), over.get("ema", ema)
    return DP.network_after_exchange(th, m, v, t, ema, reference["ranks"] if ranks is None else ranks, net, **kw)


def test_builder_is_the_update_chain_of_the_concatenated_batch(reference, stepped):
    """network_update on the concatenated batch's gradients at grad_scale 1 against the builder on the ranks' (their sum at 1 / 2):
    the same state at float64 rounding, the same decision."""
    state, bound = stepped
    whole = reference["whole"]
    for net in ("Gab", "Da"):
        th, m, v, t, ema, _ = state[net]
        g = dict(whole["grads"][net])
        sp = None
        if whole["scaled"].get(net) is not None:
            g.update({n + "_w": whole["scaled"][net][n] for n in S.LAYERS})
            sp = (th, whole["U"][net], whole["V"][net], whole["sigma"][net])
        exp = CO.network_update(th, g, m, v, t, ema, lr=LR[net], max_norm=bound, sched=SCHED, spectral=sp,
                                ema_decay=EMA_DECAY if net == "Gab" else None)
        got = _second(reference, stepped, net)
        assert got[3] == exp[3] == 2 and not got[5]["skip"] and got[5]["clip"] < 1.0
        assert abs(got[5]["norm"] - exp[5]["norm"]) <= 1e-10 * exp[5]["norm"] and abs(got[5]["clip"] - exp[5]["clip"]) <= 2.0 ** -23
        for i in (0, 1, 2) + ((4,) if ema is not None else ()):
            assert all(np.abs(got[i][k] - exp[i][k]).max() <= 1e-9 for k in exp[i]), (net, i)
        assert not DP.update_beyond(got, exp)


# ---- c. planted errors -----------------------------------------------------------------------------------------------------------------
def test_rank_1_drawing_with_offset_0_is_beyond_the_bounds(reference):
    P, U, inputs, ranks = reference["P"], reference["U"], reference["inputs"], reference["ranks"]
    wrong = [ranks[0], DP.reference_rank_step(P, U, inputs, 1, 1, 0, 0, draws_of=0)]
    assert not np.array_equal(DP.reference_rows(0, 1, 1).view(np.uint32), DP.reference_rows(0, 1, 0).view(np.uint32))
    losses = [abs(a - b) / abs(b) for a, b in zip(wrong[1]["losses"], ranks[1]["losses"])]
    bad = {net: DP.grads_beyond(DP.exchanged(wrong, net), DP.exchanged(ranks, net)) for net in ("Gab", "Da")}
    print("rank 1 at offset 0: losses off by", losses, "; tensors beyond 2e-4:", {n: len(b) for n, b in bad.items()})
    assert all(e > DP.LOSS_TOL for e in losses) and all(bad.values())


def test_update_chain_errors_are_beyond_the_bounds(reference, stepped):
    """Planted errors 2-7 of the issue, each against the correct second step."""
    state, bound = stepped
    world = len(reference["ranks"])
    right = {net: _second(reference, stepped, net) for net in ("Gab", "Da")}
    found = {}

    def planted(name, net, got, expect):
        bad = DP.update_beyond(got, right[net])
        found[(name, net)] = bad
        print(f"{name} [{net}]:", bad)
        assert expect & set(bad), (name, net, bad)

    for net in ("Gab", "Da"):
        # 2. grad_scale 1 where it should be 1 / world, in the norm and in the update: with every update clipped the two cancel in
        #    theta, m and v (the clipped gradient has the bound's length either way) -- the guard's record shows it
        planted("grad_scale 1 in the update", net, _second(reference, stepped, net, grad_scale=1.0), {"norm", "clip"})
        # 3. ... in the norm only: the clip factor is 1 / world of the right one, the applied gradient with it
        got = _second(reference, stepped, net, max_norm=bound / world)
        got[5]["norm"] *= world
        planted("grad_scale 1 in the norm only", net, got, {"m", "v", "clip"})
        # 4. the norm of ONE rank's buffer, measured before the sum
        own = _second(reference, stepped, net, ranks=reference["ranks"][:1], grad_scale=1.0 / world)[5]
        got = _second(reference, stepped, net, max_norm=bound * right[net][5]["norm"] / own["norm"])
        got[5]["norm"] = own["norm"]
        planted("the norm taken before the sum", net, got, {"norm", "clip", "m"})
        # 7. Adam's t one behind
        planted("t one behind", net, _second(reference, stepped, net, t=state[net][3] - 1), {"t"})
        assert "theta" in found[("t one behind", net)]
    # 5. the spectral transform with another u (rank 1's own seeded start, had nothing made the replicas identical)
    th = state["Da"][0]
    U1, V, sigma = S.iterate(th, S.init_u(S.discriminator_param_shapes(df_dim=8), np.random.default_rng(26)))
    got = _second(reference, stepped, "Da", spectral=(th, U1, V, sigma))
    assert DP.grads_beyond(got[5]["g"], right["Da"][5]["g"])
    planted("the transform with rank 1's own u", "Da", got, {"norm", "clip", "m", "theta"})
    # 6. the average started from rank 1's own initial weights
    other = CO.case_params(np.random.default_rng(26), False)["Gab"]
    planted("the average from rank 1's own weights", "Gab", _second(reference, stepped, "Gab", ema=other), {"ema"})


# ---- d. the ambiguity caps of the GPU cases --------------------------------------------------------------------------------------------
def test_gpu_cases_stay_under_the_sign_cap(cycle, featmatch):
    (rA, sA, _), (rB, sB, _) = cycle["inputs"]
    elements, ambiguous = CO.sign_counts(cycle["raw"], rA, rB, sA, sB)
    print(f"cycle case: {ambiguous} of {elements} sign() arguments within 1e-4 of zero")
    assert elements > 0 and ambiguous <= CAP * elements
    for r in range(2):                                  # ... and on each rank's rows alone
        (a, sa, _), (b, sb, _) = (DP.rows_of(x, r, 1) for x in cycle["inputs"])
        e, amb = CO.sign_counts(cycle["ranks"][r]["images"], a, b, sa, sb)
        assert e > 0 and amb <= CAP * e, (r, amb, e)
    for r in [featmatch["whole"]] + featmatch["ranks"]:
        e, amb, _ = FM.sign_counts(r["features"], FM.MARGIN)
        print(f"feature-matching case: {amb} of {e} sign() arguments within 1e-4 of zero")
        assert e > 0 and amb <= FM.CAP * e == CAP * e


# ---- the harness's own rules that need no device -------------------------------------------------------------------------------------
def test_harness_starts_nothing_beyond_two_workers_or_after_a_lost_worker(monkeypatch):
    from tests import dp_harness
    with pytest.raises(AssertionError, match="at most 2 workers"):
        dp_harness.launch(print, [None] * 3)
    monkeypatch.setattr(dp_harness, "_POISONED", "a worker was ended by signal 9")
    with pytest.raises(AssertionError, match="nothing was started"):
        dp_harness.launch(print, [None, None])
    assert dp_harness.LAUNCH_LIMIT_S == 3 * dp_harness.MEASURED_LAUNCH_S
