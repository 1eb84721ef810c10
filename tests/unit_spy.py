"""Recorder for the layer units of module.py and the runner that holds every recorded call to tests/unit_oracle.py.

``Spy(walk)`` is a context manager: for every unit of ``walk.conv_units()`` (a network's _ConvUnits or a lockstep pair's
_PairUnits) it puts a wrapper in place of the INSTANCE's ``forward`` and ``backward`` -- the walks call exactly these -- which
calls through and keeps the arguments and results, every tensor copied to the host at call time (buffers are reused, dropout
masks in place).  A backward call also notes whether the record it was handed is one that THIS unit's forward returned: the
per-unit reference is evaluated on the record the call got, so a record handed to the wrong backward would otherwise be
consistent with itself.  On exit it restores the units and keeps the networks' gradient buffers as the pass left them."""
import numpy as np
import torch

from tests import unit_oracle as UO


def rec(t):
    """A device tensor -> unit_oracle.Rec (float32 values are exact for both storage types), None -> None."""
    if t is None:
        return None
    name = {torch.bfloat16: "bf16", torch.float32: "f32"}[t.dtype]
    return UO.Rec(t.detach().to(torch.float32).cpu().numpy().copy(), name)


class Spy:
    def __init__(self, walk, route_name=None):
        """route_name: the package's ``_abi.route_name`` -- a backward call then keeps the name of its data-gradient route."""
        self.walk, self.route_name = walk, route_name
        self.units = list(walk.conv_units())
        self.calls = []                      # ("forward" | "backward", unit, dict) in call order
        self.records = {}                    # id(unit) -> the records its forwards returned (a backward must be handed one of them)
        self.grads = None

    def nets(self, u):
        """[(network, its unit)]: one entry for a _ConvUnit, the two halves of a _PairUnit."""
        return [(u.ua.net, u.ua), (u.ub.net, u.ub)] if hasattr(u, "ua") else [(u.net, u)]

    def _drop(self, u, drop):
        """drop = (stream id, sample offset) -> per network (stream, offset, step, seed, rate), read when the launch is queued."""
        if drop is None:
            return None
        return [(int(drop[0]), int(drop[1]), int(net.P.iterations.item()), int(net.seed), float(net.dropout)) for net, _ in self.nets(u)]

    def _wrap(self, u):
        fwd, bwd = u.forward, u.backward
        spy = self

        def forward(x, residual=None, record_only=False, out=None, drop=None):
            y, r = fwd(x, residual=residual, record_only=record_only, out=out, drop=drop)
            g = r[0]
            spy.records.setdefault(id(u), []).append(r)
            spy.calls.append(("forward", u, dict(x=rec(x), residual=rec(residual), record_only=bool(record_only), xc=rec(r[2]), stats=rec(r[3]),
                                                 y=rec(y) if u.norm else None, drop=spy._drop(u, drop), stats_chunks=int(g.stats_chunks))))
            return y, r

        def backward(r, dy, want_dx=True, param_grads=True, gbuf=None, addend=None, dy_partial=None, next_norm=None):
            g, x, xc, stats, *rest = r
            y = rest.pop(0) if u.skip_grad else None
            drop = rest[0] if rest else None
            d = dict(x=rec(x), xc=rec(xc), stats=rec(stats), y=rec(y), dy=rec(dy), addend=rec(addend), drop=spy._drop(u, drop),
                     param_grads=bool(param_grads), had_dy_partial=dy_partial is not None,
                     dgrad_route=spy.route_name(g.route_dgrad) if spy.route_name is not None else None,
                     bwd_stats_chunks=int(g.bwd_stats_chunks), dx=None, dskip=None, partial=None, next=None,
                     own_record=any(r is k for k in spy.records.get(id(u), ())))
            res = bwd(r, dy, want_dx, param_grads, gbuf, addend=addend, dy_partial=dy_partial, next_norm=next_norm)
            dx = res
            if u.skip_grad:
                dx, dskip = res
                d["dskip"] = rec(dskip)
            elif next_norm is not None:
                dx, partial = res
                d["partial"] = rec(partial)
                if partial is not None:
                    nu, nrec = next_norm
                    d["next"] = (UO.layer_of(nu), rec(nrec[2]), rec(nrec[3]), nu.name)
            d["dx"] = rec(dx)
            spy.calls.append(("backward", u, d))
            return res

        u.forward, u.backward = forward, backward

    def __enter__(self):
        for u in self.units:
            self._wrap(u)
        return self

    def __exit__(self, *exc):
        for u in self.units:
            del u.forward, u.backward
        nets = {id(net): net for u in self.units for net, _ in self.nets(u)}
        self.grads = {k: net.P.export(net.P.grad) for k, net in nets.items()}
        self.params = {k: net.P.export() for k, net in nets.items()}
        return False


def _slice(call, sl, half):
    """One network's images of a recorded call."""
    out = {}
    for k, v in call.items():
        if isinstance(v, UO.Rec):
            out[k] = UO.Rec(v.a[sl], v.name)
        elif k == "drop" and v is not None:
            out[k] = v[half]
        else:
            out[k] = v
    return out


def check(spy, dtype_name, report=None, only_net=None):
    """Every recorded call against the float64 unit -> [(unit name, network index, kind, Stage)] of all stages; ``report``: a
    dict stage -> worst ratio, updated in place.  only_net: of a lockstep pair, check this network's images and gradients alone."""
    results = []
    parts = {}
    P = {k: UO.quantised_params(v, dtype_name) for k, v in spy.params.items()}
    for kind, u, call in spy.calls:
        L = UO.layer_of(u)
        nets = spy.nets(u)
        n = call["x"].a.shape[0] // len(nets)
        for half, (net, _) in enumerate(nets):
            if only_net is not None and half != only_net:
                continue
            sl = slice(half * n, (half + 1) * n) if len(nets) > 1 else slice(None)
            c = _slice(call, sl, half)
            if kind == "forward":
                stages = UO.check_forward(L, P[id(net)], c, eps=net.eps)
            else:
                if c["next"] is not None:
                    nL, nxc, nst, nname = c["next"]
                    q = P[id(net)]
                    c["next"] = (nL, UO.Rec(nxc.a[sl], nxc.name), UO.Rec(nst.a[sl], nst.name), q[nname + "_g"], q[nname + "_beta"])
                if c["partial"] is not None:
                    c["partial"] = UO.Rec(call["partial"].a[sl], "f32")
                stages, p = UO.check_backward(L, P[id(net)], c, eps=net.eps)
                parts.setdefault((id(net), half, L), []).append(p)
            results += [(L.name, half, kind, s) for s in stages]
    for (net_id, half, L), plist in parts.items():
        G = spy.grads[net_id]
        grads = {"dw": G[L.name + "_w"], "db": G[L.name + "_b"]}
        if L.norm:
            grads.update(dgamma=G[L.name + "_g"], dbeta=G[L.name + "_beta"])
        results += [(L.name, half, "grads", s) for s in UO.check_param_grads(L, plist, grads)]
    if report is not None:
        for _, _, kind, s in results:
            key = f"{kind}.{s.stage}"
            report[key] = max(report.get(key, 0.0), s.ratio)
            report["kink fraction"] = max(report.get("kink fraction", 0.0), s.kinks)
    return results


def failures(results):
    return [f"{name}[net {half}] {kind}.{s.stage}: ratio {s.ratio:.3g} at {s.index}: got {s.got!r}, reference {s.ref!r}, |err| {s.err:.3g} > bound {s.bound:.3g}"
            f" (kink fraction {s.kinks:.2g})" for name, half, kind, s in results if not (s.ratio <= 1.0 and s.kinks <= UO.KINK_FRACTION)]
