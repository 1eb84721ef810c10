"""The world-2 data-parallel step with the options on, two ranks sharing the one device (tests/dp_harness.py), against
tests/dp_oracle.py: what the options claim about data parallelism -- a rank draws the single-device run's rows of ITS samples, the
guard measures the exchanged buffer at 1 / world, the spectral transform runs once on that buffer, every rank keeps the same
average -- and what all of it rests on: enable_data_parallel() leaves the replicas identical in everything state_dict() writes
and in their draw keys.

f32 models of tests/test_gpu_composed.py's size (ngf = ndf = 8, 128 x 128, SCHED), parameters and inputs from
composed_oracle.case_params / case_inputs, bounds the single-process files' own, unchanged (dp_oracle.LOSS_TOL .. U32): losses
2e-5, every gradient tensor 2e-4 in relative L2 and worst entry over largest, u within U_BOUND, the update 2e-6, the average
3 * 2^-24 of its largest entry (+ the update's 2e-6), draws, zero patterns and everything replica-against-replica bitwise.

One launch per case; inside it the eager model steps first, then the graph=True model from the same start.  The eager steps are
held to float64 (the oracle runs inside the workers, after their last collective, the two ranks' in parallel); the replayed steps
are held to the eager ones BIT FOR BIT -- losses, draws, images, every exchanged buffer, every piece of state -- which hands every
bound the eager steps meet on to them, and needs no forward records of a captured step.

How the update is compared.  Adam divides by |g|: a parameter whose gradient lies within the kernels' rounding of zero moves by
up to the rate, whichever sign the rounding leaves.  So theta, m, v and the average are compared at 2e-6 with
dp_oracle.network_after_exchange going on from the buffer the update really read (tests/test_gpu_composed.py's update-chain test
does the same), and that buffer is held to the float64 sum of the two ranks' oracle gradients, and the guard's record to the norm
and clip factor of that float64 sum, at the gradients' 2e-4."""
import hashlib

import numpy as np
import pytest
import torch

from tests import composed_oracle as CO
from tests import dp_harness
from tests import dp_oracle as DP
from tests import spectral_oracle as S

pytestmark = pytest.mark.gpu

H = W = DP.H
WORLD = DP.WORLD
# the float64 oracle of ONE step on one sample inside a worker, in seconds of CPU, doubled for a loaded machine (measured without a
# GPU: the reference step 10 s at N = 2, the cycle step 29 s; the two ranks' run in parallel)
REFERENCE_ORACLE_S, CYCLE_ORACLE_S = 15.0, 30.0


# ---- inside a worker -----------------------------------------------------------------------------------------------------------------
def _digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _replicated(m):
    """Digests of everything the replicas must agree on bit for bit: what state_dict() writes (parameters, slots, counter, the
    guard's record, the average and its factors, u) and the exchanged gradient buffers."""
    out = {}
    for name, net in zip(m._net_names(), m.networks()):
        P = net.P
        for k, t in (("flat", P.flat), ("m", P.m), ("v", P.v), ("t", P.iterations), ("grad", P.grad), ("guard", P._guard),
                     ("ema", P.ema), ("ema_state", P._ema_state), ("u", net.spectral_state())):
            if t is not None:
                out[f"{name}.{k}"] = _digest(t)
    return out


def _per_rank(m):
    """... and of what belongs to the rank: its losses, its images, its drawn table."""
    out = {"loss": _digest(m._loss), "fake_A": _digest(m.fake_A.tensor())}
    if m.diffaug:
        out["table"] = _digest(m.diffaug_params)
    return out


def _state_dict_host(m):
    out = {}
    for key, entry in m.state_dict().items():
        for k, v in entry.items():
            out[f"{key}.{k}"] = v.numpy().copy() if isinstance(v, torch.Tensor) else v
    return out


def _keys(m):
    Ds = [n for n in m.networks() if n.spectral_state() is not None]
    return {"seeds": [n.seed for n in m.networks()], "diffaug": m._diffaug_seed, "u0": [D._sn.u0.numpy().copy() for D in Ds]}


def _model_kw(case):
    from tests.test_gpu_composed import ALL
    kind = case["kind"]
    if kind == "featmatch":
        from tests import featmatch_oracle as FO
        return dict(ngf=8, ndf=8, n_blocks=1, dtype="f32", d_quad=True, fm_lambda=FO.FM_LAMBDA, use_resnet=True, d_norm="spectral",
                    ssim_lambda=CO.SSIM_LAMBDA, skip_nonfinite=True, lr_decay=True)
    kw = dict(ALL, dtype="f32")
    if kind == "cycle":
        kw.update(cycle=True, paired=case.get("paired"))
    else:
        kw.update(d_quad=True)
    return kw


def _case_data(case):
    n, steps = case.get("n", 1), case.get("steps", 2)
    if case["kind"] == "cycle":
        P, inputs = DP.cycle_case(steps, n * WORLD)
        return P, None, inputs
    if case["kind"] == "featmatch":
        P, U, inputs = DP.featmatch_case(n * WORLD)
        return P, U, [inputs] * steps
    P, inputs = DP.reference_case(steps, n * WORLD)
    return P, None, inputs


def _feed(m, case, inputs, step, rank, poison=False):
    from tests.test_gpu_composed import _poison
    n = case.get("n", 1)
    if m.cycle:
        (rA, sA, mA), (rB, sB, mB) = (DP.rows_of(x, rank, n) for x in inputs[step])
        m.real_A, m.seg_A, m.mask_A, m.real_B, m.seg_B, m.mask_B = rA, sA, mA, rB, sB, mB
    else:
        m.real_A, m.seg_A, m.mask_A = DP.rows_of(inputs[step], rank, n)
    if poison:
        m.real_A = _poison(m.real_A)


def _probe_clip(sg, case, kw, P, inputs, rank):
    """tests/test_gpu_composed._model's rule, data parallel: a probe step without a bound, then a quarter of the smallest norm the
    guard recorded -- measured after the exchange, so both ranks read the same bits (the parent checks that)."""
    from tests.test_gpu_composed import _build, _load
    probe = _build(sg, 1e30, **dict(kw, graph=False, keep_tapes=False))
    _load(probe, P)
    probe.enable_data_parallel()
    _feed(probe, case, inputs, 0, rank)
    probe.train_step()
    norms = {k: st["norm"] for k, st in probe.grad_stats().items()}
    assert all(0.0 < v < float("inf") for v in norms.values()), norms
    return 0.25 * min(norms.values()), norms


def _export32(net, buf=None):
    return {k: v.copy() for k, v in net.P.export(buf).items()}


def _pre_state(nets):
    from tests.test_gpu_composed import _export
    from tests.test_gpu_spectral import _u_of
    return {n: {"theta": _export(net), "m": _export(net, net.P.m), "v": _export(net, net.P.v), "t": net.P.step_count,
                "ema": None if net.P.ema is None else _export(net, net.P.ema),
                "U": None if net.spectral_state() is None else _u_of(net)} for n, net in nets.items()}


def _tap_pre_transform(m, nets, snaps):
    """Keep a copy of every spectral discriminator's exchanged buffer as it is directly before the transform (eager steps only)."""
    for n, net in nets.items():
        if net.spectral_state() is not None:
            def tapped(gbuf=None, net=net, n=n, real=net.spectral_grad):
                snaps[n] = net.P.grad.clone()
                return real(gbuf)
            net.spectral_grad = tapped


def _oracle_worker(rank, world, case):
    """One rank of the cases c .. f.  Phase 1, on the device: the eager model's steps (forward records read, states exported),
    then the graph=True model's, compared with the eager ones bit for bit.  Phase 2, after the last collective: the float64 oracle of
    every eager step on this rank's rows and the comparisons that need nothing of the other rank."""
    import sggan_amd as sg
    import torch.distributed as dist
    from tests import unet_cycle_oracle as UC
    from tests import unet_oracle as UO
    from tests.kink_helpers import discriminator_branches, generator_branches
    from tests.test_gpu_composed import SCHED, _build, _cycle_tape_masks, _kept_bits, _load, _nets, _table, _zero_pattern
    from tests.test_gpu_spectral import U_BOUND, _kinked, _u_of
    kind, n, steps = case["kind"], case.get("n", 1), case.get("steps", 2)
    poisoned = case.get("poison_step")                      # (rank 1's real_A carries one NaN at this step)
    oracle = case.get("oracle", True)
    P, _, inputs = _case_data(case)                         # (u: the device's own seeded start, as tests/test_gpu_featmatch.py takes it)
    kw = _model_kw(case)
    clip, norms = _probe_clip(sg, case, kw, P, inputs, rank)
    out = {"clip": clip, "probe_norms": norms, "failures": [], "steps": [], "graph": []}
    fail = out["failures"].append
    todo = []

    # ---- phase 1 ----
    for graph in (False, True):
        cycle = kind == "cycle"
        paired = bool(case.get("paired")) if cycle else False
        tapes = not graph and (not cycle or paired)
        m = _build(sg, clip, graph=graph, keep_tapes=tapes, **kw)
        _load(m, P)
        m.enable_data_parallel()
        nets = _nets(m)
        twin = None
        if not graph and cycle and not paired and oracle:
            # the one-network-at-a-time step keeps no forward records: the kink decisions and the zero patterns are read from a
            # lockstep twin that takes the same step from the same state (tests/test_gpu_composed.py's device) -- data parallel
            # too, so that it draws at this rank's offset; both ranks step their twins, so the collectives pair up
            twin = _build(sg, clip, keep_tapes=True, d_quad=False, **dict(kw, paired=True))
            twin.enable_data_parallel()
        snaps = {}
        if not graph:
            _tap_pre_transform(m, nets, snaps)
        for step in range(steps):
            bad = poisoned == step and rank == 1
            pre = _pre_state(nets) if not graph and oracle else None
            kept = _kept_bits(m)
            t = {k: net.P.step_count for k, net in nets.items()}
            if twin is not None:
                for net, tn in zip(nets.values(), _nets(twin).values()):
                    tn.P.load(net.P.export())
                    tn.P.step_count = net.P.step_count
                    if tn.spectral_state() is not None:
                        tn.set_spectral_state(net.spectral_state())
                _feed(twin, case, inputs, step, rank)
                twin.train_step()
            _feed(m, case, inputs, step, rank, poison=bad)
            fm_dev = None
            if kind == "featmatch" and not graph:
                from tests.test_gpu_featmatch import _Tap
                with _Tap(sg.kernels) as tap:
                    m.train_step()
                fm_dev = tap.calls[0]
            else:
                m.train_step()
            rec = {"replicated": _replicated(m), "own": _per_rank(m), "losses": m.losses(), "stats": m.grad_stats(), "t": t,
                   "kept": {k: [torch.equal(a, b) for a, b in zip(kept[k], v)] for k, v in _kept_bits(m).items()},
                   "finite": {k: bool(torch.isfinite(net.P.grad).all()) for k, net in zip(m._net_names(), m.networks())}}
            if m.diffaug:                                   # the draws: this rank's rows of the single-device run's, both variants
                rows = DP.cycle_rows(t["Da"], t["Db"], n, rank, seed=m._diffaug_seed) if cycle else DP.reference_rows(t["Da"], n, rank, seed=m._diffaug_seed)
                if not np.array_equal(_table(m), rows.view(np.uint32)):
                    fail(f"graph={graph} step {step}: the drawn table is not this rank's rows")
                rec["table"] = _table(m).copy()
            if graph:
                out["graph"].append(rec)
                continue
            source = twin if twin is not None else m
            if m.dropout is not None and (tapes or twin is not None):
                try:                                        # the zero patterns of d1..d3's recorded pre-norm tensors
                    if cycle:
                        _cycle_tape_masks(source, DP.cycle_masks(t["Gab"], t["Gba"], n, rank, seed=m.generator.seed), n)
                    else:
                        _zero_pattern([m.tapes["G"][8 + l][2] for l in range(3)], DP.generator_masks(t["Gab"], m.generator.seed, 0, n, rank), "G")
                except AssertionError as e:
                    fail(f"step {step}: zero pattern: {e}")
            if oracle and not bad and poisoned != step:
                if cycle:
                    br = UC.unet_cycle_step_branches(source)
                    images = {k: getattr(m, k).numpy().astype(np.float64) for k in ("fake_A", "fake_B", "cyc_A", "cyc_B")}
                else:
                    G, D, tp = m.generator, m.discriminator, m.tapes
                    gen = generator_branches(G, tp["G"]) if kind == "featmatch" else UO.unet_branches(G, tp["G"])
                    br, images = gen + discriminator_branches(D, tp["D_real"]) + discriminator_branches(D, tp["D_fake"]), None
                rec["buffer"] = {k: _export32(net, snaps.get(k, net.P.grad)) for k, net in nets.items()}      # exchanged, before any transform
                rec["grad"] = {k: _export32(net, net.P.grad) for k, net in nets.items()}          # ... and as the update read it
                post = _pre_state(nets)
                todo.append((step, rec, pre, post, br, images, fm_dev, t))
            out["steps"].append(rec)
        del m, twin
    dist.barrier()

    # ---- phase 2 ----
    for k, (e, g) in enumerate(zip(out["steps"], out["graph"])):
        for part in ("replicated", "own"):
            differ = [key for key in e[part] if e[part][key] != g[part][key]]
            if differ:
                fail(f"step {k}: the replayed step differs from the eager one in {differ}")
        if repr(e["stats"]) != repr(g["stats"]):            # (repr: a skipped update records a non-finite norm)
            fail(f"step {k}: the guard records of the replayed step differ: {g['stats']} {e['stats']}")
    lr = sg.sggan.LR if kind != "cycle" else kw.get("lr", 0.0002)
    for step, rec, pre, post, br, images, fm_dev, t in todo:
        Pn = {k: s["theta"] for k, s in pre.items()}
        if kind == "cycle":
            sp = S.SignPolicy(1e-4, images)
            r = _kinked(br, lambda: DP.cycle_rank_step(Pn, pre["Da"]["U"], pre["Db"]["U"], *inputs[step], rank, n, t, signs=sp))
            if not (sp.disagree_outside == 0 and sp.ambiguous <= 5e-3 * sp.elements):
                fail(f"step {step}: signs {sp.ambiguous} of {sp.elements} ambiguous, {sp.disagree_outside} disagree outside the margin")
        elif kind == "featmatch":
            sp = S.SignPolicy(1e-4)
            r = _kinked(br, lambda: DP.featmatch_rank_step(Pn, pre["Da"]["U"], inputs[step], rank, n, signs=sp, dev=fm_dev))
            if not (sp.disagree_outside == 0 and sp.ambiguous <= 5e-3 * sp.elements):
                fail(f"step {step}: signs {sp.ambiguous} of {sp.elements} ambiguous, {sp.disagree_outside} disagree outside the margin")
        else:
            r = _kinked(br, lambda: DP.reference_rank_step(Pn, pre["Da"]["U"], inputs[step], rank, n, t["Gab"], t["Da"]))
        rec["oracle"] = {k: r[k] for k in ("losses", "grads", "scaled")}
        if rank == 0:                                       # (the replicas' states are the same bits: one copy is enough)
            rec["before"] = {"P": Pn, "U": {k: s["U"] for k, s in pre.items() if s["U"] is not None}}
        for net in pre:
            ema_decay = 0.999 if pre[net]["ema"] is not None else None
            if r["U"].get(net) is not None:
                worst_u = max(float(np.abs(post[net]["U"][l] - r["U"][net][l]).max()) for l in S.LAYERS)
                if not worst_u <= U_BOUND:
                    fail(f"step {step} {net}: u off by {worst_u}")
                # the transform: the device's transformed buffer against the float64 transform of the device's exchanged one
                pre_t, got = {k: v.astype(np.float64) for k, v in rec["buffer"][net].items()}, rec["grad"][net]
                exp = dict(pre_t)
                for l in S.LAYERS:
                    exp[l + "_w"] = S.grad_transform(pre_t[l + "_w"], Pn[net][l + "_w"], r["U"][net][l], r["V"][net][l], 1.0 / r["sigma"][net][l])
                beyond = DP.grads_beyond(got, exp)
                if beyond:
                    fail(f"step {step} {net}: the transform of the exchanged buffer: {beyond}")
            # the update chain, once, from the buffer the update read, at grad_scale 1 / world
            s0, s1, stats = pre[net], post[net], rec["stats"][{"Gab": "G", "Da": "D", "Gba": "G_BA", "Db": "D_B"}[net]]
            exp = DP.network_after_exchange(s0["theta"], s0["m"], s0["v"], s0["t"], s0["ema"], [r] * world, net, lr=lr, max_norm=clip,
                                            sched=SCHED, ema_decay=ema_decay, buffer={k: v.astype(np.float64) for k, v in rec["grad"][net].items()})
            got = (s1["theta"], s1["m"], s1["v"], s1["t"], s1["ema"], {"norm": stats["norm"], "clip": stats["clip"], "skip": False})
            beyond = DP.update_beyond(got, exp)
            if beyond or not abs(stats["norm"] - exp[5]["norm"]) <= 1e-12 * exp[5]["norm"] or stats["clip"] != exp[5]["clip"]:
                fail(f"step {step} {net}: the update: {beyond}, record {stats}, expected norm {exp[5]['norm']!r} clip {exp[5]['clip']!r}")
    return out


# ---- in the parent -------------------------------------------------------------------------------------------------------------------
def _no_failures(res):
    for r in res:
        assert not r["failures"], (r["rank"], r["failures"])


def _replicas_agree(res, steps):
    """Everything replicated is the same bits on both ranks after every step of both variants; what belongs to a rank differs."""
    for variant in ("steps", "graph"):
        for k in range(steps):
            a, b = res[0][variant][k], res[1][variant][k]
            differ = [key for key in a["replicated"] if a["replicated"][key] != b["replicated"][key]]
            assert not differ and set(a["replicated"]) == set(b["replicated"]), (variant, k, differ)
            assert repr(a["stats"]) == repr(b["stats"]), (variant, k, a["stats"], b["stats"])
            assert a["own"]["loss"] != b["own"]["loss"] and a["own"]["fake_A"] != b["own"]["fake_A"], (variant, k)
            if "table" in a:
                assert not np.array_equal(a["table"], b["table"]), (variant, k)


def _check_against_oracle(res, steps, nets, concatenated=None):
    """Per step and rank: the rank's losses against its oracle's; the exchanged buffer -- a spectral discriminator's before the
    transform -- against the sum of the two ranks' oracle gradients, and after it against the sum of their gradients with respect
    to W; the guard's record against the norm of that sum at 1 / world; every update clipped and counted alike; the mean of the
    ranks' losses against the mean of the ranks' oracle losses, which is the concatenated batch's (tests/test_dp_oracle_cpu.py, at
    1e-11, for these inputs) -- and against ``concatenated(step, P, U, t)``, the oracle on the concatenated batch itself, where a
    test hands one in (the reference steps; the cycle step's costs as much as the rest of its test and is left to the CPU file)."""
    assert res[0]["clip"] == res[1]["clip"] and res[0]["probe_norms"] == res[1]["probe_norms"], "the probe's norms differ between the ranks"
    clip = res[0]["clip"]
    names = {"Gab": "G", "Da": "D", "Gba": "G_BA", "Db": "D_B"}
    for k in range(steps):
        ranks = [res[r]["steps"][k]["oracle"] for r in range(WORLD)]
        for r in range(WORLD):
            rec = res[r]["steps"][k]
            for got, exp in zip(rec["losses"], ranks[r]["losses"]):
                assert abs(got - exp) < DP.LOSS_TOL * abs(exp), (k, r, rec["losses"], ranks[r]["losses"])
            for net in nets:
                summed = DP.exchanged(ranks, net)
                w = DP.worst(rec["buffer"][net], summed)
                print(f"step {k + 1} rank {r} {net}: exchanged buffer, worst", sorted(w.items(), key=lambda kv: -max(kv[1]))[:2])
                assert len(w) == 16 if net[0] == "D" else len(w) >= 20, (net, len(w))      # (D: every tensor, the biases included)
                assert all(np.abs(rec["buffer"][net][key]).max() < 1e-6 for key in summed if key not in w), net
                assert not DP.grads_beyond(rec["buffer"][net], summed), (k, r, net, DP.grads_beyond(rec["buffer"][net], summed))
                wrt_w = {key: sum(x["grads"][net][key] for x in ranks) for key in ranks[0]["grads"][net]}
                assert not DP.grads_beyond(rec["grad"][net], wrt_w), (k, r, net, DP.grads_beyond(rec["grad"][net], wrt_w))
                norm = float(np.sqrt(sum((np.asarray(v, np.float64) ** 2).sum() for v in wrt_w.values()))) / WORLD
                st = rec["stats"][names[net]]
                assert abs(st["norm"] - norm) <= DP.GRAD_TOL * norm, (k, r, net, st, norm)
                assert st["clip"] < 1.0 and abs(st["clip"] - clip / norm) <= DP.GRAD_TOL * clip / norm + 2.0 ** -24, (k, r, net, st, clip / norm)
                assert (st["skipped"], st["applied"]) == (0, k + 1), (k, r, net, st)
        mean = np.mean([res[r]["steps"][k]["losses"] for r in range(WORLD)], axis=0)
        for got, exp in zip(mean, DP.mean_losses(ranks)):
            assert abs(got - exp) < DP.LOSS_TOL * abs(exp), (k, got, exp)
        if concatenated is not None:
            before = res[0]["steps"][k]["before"]
            whole = concatenated(k, before["P"], before["U"], res[0]["steps"][k]["t"])
            print(f"step {k + 1}: mean of the ranks' losses {tuple(mean)}, the concatenated batch's oracle {whole}")
            for got, exp in zip(mean, whole):
                assert abs(got - exp) < DP.LOSS_TOL * abs(exp), (k, got, exp)


# ---- a. replicas are made identical ----------------------------------------------------------------------------------------------------
def _identical_worker(rank, world, case):
    import sggan_amd as sg
    from tests.test_gpu_composed import ALL, _build, _table
    kw = dict(ALL, dtype="f32", cycle=True)
    _, inputs = DP.cycle_case(2, WORLD)
    out = {"variants": []}
    donor_sd = None
    if rank == 0:                                           # a state that is nobody's initialisation: three steps of another model
        donor = _build(sg, 1.0, seed=5, **kw)
        rng = np.random.default_rng(77)
        for _ in range(3):
            donor.real_A, donor.seg_A, donor.mask_A = CO.case_inputs(rng, 1)
            donor.real_B, donor.seg_B, donor.mask_B = CO.case_inputs(rng, 1)
            donor.train_step()
        donor_sd = donor.state_dict()
        out["donor"] = {"t": [n.P.step_count for n in donor.networks()], "stats": donor.grad_stats(),
                        "ema_moved": [not torch.equal(n.P.ema, n.P.flat) for n in donor._ema_nets()]}
        del donor
    for graph in (False, True):
        m = _build(sg, 1.0, seed=19 + 7 * rank, graph=graph, **kw)
        if rank == 0:
            m.load_state_dict(donor_sd)
        rec = {"built": _keys(m)}
        m.enable_data_parallel()
        rec.update(keys=_keys(m), state=_state_dict_host(m), steps=[])
        for step in range(2):
            t = {"Da": m.discriminator.P.step_count, "Db": m.discriminator_B.P.step_count}
            _feed(m, {"kind": "cycle"}, inputs, step, rank)
            m.train_step()
            rows = DP.cycle_rows(t["Da"], t["Db"], 1, rank, seed=m._diffaug_seed).view(np.uint32)
            rec["steps"].append({"replicated": _replicated(m), "stats": m.grad_stats(), "table": _table(m).copy(),
                                 "table_is_own_rows": bool(np.array_equal(_table(m), rows)), "t": t})
        rec["after"] = _state_dict_host(m)
        out["variants"].append(rec)
        del m
    return out


def _same_bits(a, b):
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def test_enable_data_parallel_makes_the_replicas_identical():
    """Rank r is built with seed 19 + 7 r, every option on, cycle mode; rank 0 then loads the state of a model that has stepped
    three times (slots non-zero, counters at 3, the average off the parameters, u moved, the guard's counters non-zero).  After
    enable_data_parallel() every key of state_dict() is the same bits on both ranks, and so are the draw keys and the seeded start
    of u; after two steps on different halves of a batch they still are, with the exchanged buffers and the guard's records, while
    each rank's drawn table is its own rows of the single-device run's and differs from the other's."""
    res = dp_harness.launch(_identical_worker, [None, None], models=3)
    print("transport:", res[0]["transport"])
    donor = res[0]["donor"]
    assert donor["t"] == [3, 3, 3, 3] and all(donor["ema_moved"]) and all(v["applied"] == 3 for v in donor["stats"].values()), donor
    for a, b in zip(res[0]["variants"], res[1]["variants"]):
        assert a["built"]["seeds"] != b["built"]["seeds"] and a["built"]["diffaug"] != b["built"]["diffaug"]   # (they were built apart)
        assert a["keys"]["seeds"] == b["keys"]["seeds"] == a["built"]["seeds"] and a["keys"]["diffaug"] == b["keys"]["diffaug"] == 19
        assert len(a["keys"]["u0"]) == 2 and all(np.array_equal(x, y) for x, y in zip(a["keys"]["u0"], b["keys"]["u0"]))
        for when in ("state", "after"):
            assert set(a[when]) == set(b[when]) and any(k.endswith(".ema") for k in a[when]) and any(k.endswith(".u") for k in a[when])
            differ = [k for k in a[when] if not _same_bits(a[when][k], b[when][k])]
            assert not differ, (when, differ)
        assert all(a["state"][f"{k}.t"] == 3 for k in ("G", "D", "G_BA", "D_B")) and all(a["after"][f"{k}.t"] == 5 for k in ("G", "D", "G_BA", "D_B"))
        assert all(a["state"][f"{k}.guard"] == [0, 3] for k in ("G", "D", "G_BA", "D_B")), a["state"]["G.guard"]
        for x, y in zip(a["steps"], b["steps"]):
            differ = [k for k in x["replicated"] if x["replicated"][k] != y["replicated"][k]]
            assert not differ and x["stats"] == y["stats"], (differ, x["stats"], y["stats"])
            assert x["table_is_own_rows"] and y["table_is_own_rows"] and not np.array_equal(x["table"], y["table"])
    # ... and the replayed run is the eager run
    for r in res:
        e, g = r["variants"]
        assert not [k for k in e["after"] if not _same_bits(e["after"][k], g["after"][k])]


# ---- b. the rows each rank draws -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["reference", "cycle"])
def test_each_rank_draws_its_rows_of_the_single_device_run(kind):
    """Two samples per rank, global batch 4, dropout and the augmentation on, two steps, eager and replayed: rank r's table is
    rows [2r, 2r + 2) of every stream of the single-device run's at N = 4, and the zero patterns of d1..d3's recorded pre-norm
    tensors are those rows of generator_masks (checked in the workers, bitwise; the replayed steps' images, losses and buffers are
    the eager ones' bit for bit, which covers their masks).  No gradient oracle."""
    res = dp_harness.launch(_oracle_worker, [dict(kind=kind, n=2, steps=2, oracle=False, paired=True)] * WORLD, models=3)
    _no_failures(res)
    _replicas_agree(res, 2)
    for step in range(2):
        whole = (CO.cycle_rows(step, step, 4, H, W) if kind == "cycle" else CO.reference_rows(step, 4, H, W)).view(np.uint32)
        streams = len(whole) // 4
        for r in range(WORLD):
            mine = np.concatenate([whole[4 * s + 2 * r:4 * s + 2 * r + 2] for s in range(streams)])
            for variant in ("steps", "graph"):
                assert np.array_equal(res[r][variant][step]["table"], mine), (step, r, variant)
        # (generator_masks at N = 4, rows [2r, 2r + 2), is what the workers compared against: the same function of the global index)
        for l, whole_mask in enumerate(CO.generator_masks(step, CO.SEED, 0, 4, H, W, DP.C8)):
            for r in range(WORLD):
                assert np.array_equal(whole_mask[2 * r:2 * r + 2], DP.generator_masks(step, CO.SEED, 0, 2, r)[l])


# ---- c. the reference step, every option on ----------------------------------------------------------------------------------------------
def test_reference_step_every_option_on_matches_the_oracle_sum():
    res = dp_harness.launch(_oracle_worker, [dict(kind="reference", steps=2)] * WORLD, models=3, oracle_s=2 * REFERENCE_ORACLE_S)
    print("transport:", res[0]["transport"])
    _no_failures(res)
    _replicas_agree(res, 2)
    _, inputs = DP.reference_case(2)

    def concatenated(k, P, U, t):
        r = CO.reference_step(P["Gab"], P["Da"], U["Da"], *inputs[k], masks=CO.generator_masks(t["Gab"], CO.SEED, 0, WORLD, H, W, DP.C8),
                              rows=CO.reference_rows(t["Da"], WORLD, H, W), ssim_lambda=CO.SSIM_LAMBDA)
        return r["gen_loss"], r["disc_loss"]
    _check_against_oracle(res, 2, ("Gab", "Da"), concatenated)


# ---- d. the cycle step, every option on --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [None, True], ids=["default_sequencing", "paired"])
def test_cycle_step_every_option_on_matches_the_oracle_sum(paired):
    """The U-Net pair one network at a time (its default) and in lockstep, where the deferred weight gradients and the bucket
    hook meet."""
    res = dp_harness.launch(_oracle_worker, [dict(kind="cycle", steps=2, paired=paired)] * WORLD, models=3 if paired else 4,
                            oracle_s=2 * CYCLE_ORACLE_S)
    _no_failures(res)
    _replicas_agree(res, 2)
    _check_against_oracle(res, 2, ("Gab", "Gba", "Da", "Db"))


# ---- e. the skip -------------------------------------------------------------------------------------------------------------------------
def test_nan_on_one_rank_skips_the_update_on_both():
    """Case c's model.  At step 2 rank 1's real_A carries one NaN (a value, not a fault): it reaches the generator's gradient on
    rank 1, the exchange carries it to rank 0, and BOTH ranks skip the generator's update -- parameters, slots, counter and
    average keep every bit, ``skipped`` grows by one on both; a network the NaN does not reach (tests/test_gpu_composed.py: D
    sees a fake that the last ReLU made finite) is updated on both.  The two ranks' records are equal throughout, and step 3, on
    clean inputs, updates both replicas and leaves them bit-identical."""
    res = dp_harness.launch(_oracle_worker, [dict(kind="reference", steps=3, poison_step=1, oracle=False)] * WORLD, models=3)
    _no_failures(res)
    _replicas_agree(res, 3)
    for r in res:
        for variant in ("steps", "graph"):
            s1, s2, s3 = r[variant]
            assert all(s1["finite"].values()) and not any(any(k) for k in s1["kept"].values()), (variant, s1["finite"], s1["kept"])
            reached = {k for k, finite in s2["finite"].items() if not finite}
            assert "G" in reached, s2["finite"]
            for k in ("G", "D"):
                before, after = s1["stats"][k], s2["stats"][k]
                if k in reached:
                    assert all(s2["kept"][k]), (variant, k, s2["kept"][k])
                    assert (after["skipped"], after["applied"]) == (before["skipped"] + 1, before["applied"]), (variant, k, after)
                else:
                    assert not any(s2["kept"][k]) and (after["skipped"], after["applied"]) == (before["skipped"], before["applied"] + 1)
                assert not any(s3["kept"][k]) and s3["stats"][k]["applied"] == after["applied"] + 1 and s3["stats"][k]["skipped"] == after["skipped"]
            assert all(s3["finite"].values())
    assert res[0]["steps"][1]["finite"] == res[1]["steps"][1]["finite"]


# ---- f. feature matching -----------------------------------------------------------------------------------------------------------------
def test_feature_matching_step_matches_the_oracle_sum():
    """The ResNet reference step with fm_lambda on, featmatch_oracle's composed case (spectral D, the SSIM term, the guard flags),
    one sample per rank: the case the option's own file left out."""
    res = dp_harness.launch(_oracle_worker, [dict(kind="featmatch", steps=1)] * WORLD, models=3, oracle_s=REFERENCE_ORACLE_S)
    _no_failures(res)
    _replicas_agree(res, 1)
    from tests import featmatch_oracle as FO
    _, _, inputs = DP.featmatch_case()

    def concatenated(k, P, U, t):
        r = FO.case_step("composed", P, U["Da"], inputs)
        return r["gen_loss"], r["disc_loss"]
    _check_against_oracle(res, 1, ("Gab", "Da"), concatenated)
