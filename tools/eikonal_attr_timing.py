#!/usr/bin/env python3
"""Launch angle, direction and spreading at eikonal-filled nodes against two yardsticks that exist without
it, in one process: rtmi_eikonal_attributes_dev on P = 32 tables of the 737 x 539 grid of tools/eikonal_timing.py
(vert_heterogeneous sampled at the nodes, 32 sources on the lines x = 4.85 and x = -1.85), the tables filled from the source ball
alone; warmed, alternating, medians of --reps device times with min and max.

Yardstick 1 is rtmi_eikonal_tangent_dev on the same tables: the launch angle's sweep walks the same diagonals with the same two
reads per node, so its time per round is expected near the tangent's, plus one pass over the nodes for dir, J and G; that is
measured, not assumed.  Yardstick 2 is the same gather and the same differences as whole-grid Jacobi iterations in plain torch,
the coefficients computed in torch from T as well (tools/eikonal_lin_timing.py's network), every node of every table at once from
the previous iterate, run until an iteration changes nothing (looked at every --check iterations, since the look is a host
sync), then one pass of differences.  Values are compared, not bits, and the largest difference is printed.

Also printed: the rounds, the launch angle's share and the node pass's share of the call, and the two floors of the sweep kernel.

    python tools/eikonal_attr_timing.py [--tables 32] [--reps 5] [--check 64] [--no-torch] [--out FILE.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.eikonal_lin_timing import jacobi, torch_network                      # noqa: E402
from tools.eikonal_timing import CLOCK, HBM, L2_ROUND_TRIP, NX, NY, series      # noqa: E402

BYTES_PER_NODE = 17                 # the value and the weight in fp64 and the code, read by every sweep


def wrap(torch, d):
    return torch.where(d > math.pi, d - 2.0 * math.pi, torch.where(d <= -math.pi, d + 2.0 * math.pi, d))


def torch_theta0(torch, net, src, grid, check, cap):
    pad = torch.nn.functional.pad
    nan = float("nan")
    gx0, gdx, nx, gy0, gdy, ny = grid
    X = gx0 + torch.arange(nx, device=src.device, dtype=torch.float64) * gdx
    Y = gy0 + torch.arange(ny, device=src.device, dtype=torch.float64) * gdy
    at = torch.atan2(Y[None, :, None] - src[:, 1, None, None], X[None, None, :] - src[:, 0, None, None])
    v0 = torch.where(net["ball"], at, torch.full_like(at, nan))
    ha, hb = net["free"] & (net["ca"] != 0), net["free"] & (net["cb"] != 0)
    w = torch.where(ha & hb, net["cb"] / (net["ca"] + net["cb"]), torch.zeros_like(net["ca"]))

    def step(v):
        vp = pad(v, (1, 1, 1, 1), value=nan)
        va = torch.where(net["east"], vp[:, 1:-1, 2:], vp[:, 1:-1, :-2])
        vb = torch.where(net["north"], vp[:, 2:, 1:-1], vp[:, :-2, 1:-1])
        ua, ub = ha & torch.isfinite(va), hb & torch.isfinite(vb)
        both = va + w * wrap(torch, vb - va)
        new = torch.where(ua & ub, both, torch.where(ua, va, torch.where(ub, vb, torch.full_like(v, nan))))
        return torch.where(net["free"], new, v0)

    def settle(step_, v):
        # NaN == NaN is false: compare the bits, as the kernel does
        return jacobi(torch, lambda u: step_(u.view(torch.float64)).view(torch.int64), v.view(torch.int64), check, cap)

    v, it, ms = settle(step, v0)
    return v.view(torch.float64), it, ms


def torch_spread(torch, net, th, n, grid):
    """J and G by the definition's differences, one pass -> (J, G, device ms)"""
    pad = torch.nn.functional.pad
    nan = float("nan")
    _, gdx, _, _, gdy, _ = grid
    a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a_.record()
    ok = net["live"] & torch.isfinite(th)
    tp, op = pad(th, (1, 1, 1, 1), value=nan), pad(ok.to(torch.uint8), (1, 1, 1, 1)).bool()

    def diff(lo, hi, ulo, uhi, h):
        z = torch.zeros_like(th)
        lo, hi = torch.where(ulo, lo, z), torch.where(uhi, hi, z)
        return torch.where(ulo & uhi, wrap(torch, hi - lo) / (2.0 * h),
                           torch.where(uhi, wrap(torch, hi - th) / h, torch.where(ulo, wrap(torch, th - lo) / h, z)))

    ddx = diff(tp[:, 1:-1, :-2], tp[:, 1:-1, 2:], op[:, 1:-1, :-2], op[:, 1:-1, 2:], gdx)
    ddy = diff(tp[:, :-2, 1:-1], tp[:, 2:, 1:-1], op[:, :-2, 1:-1], op[:, 2:, 1:-1], gdy)
    J = torch.where(net["free"] & torch.isfinite(th), 1.0 / torch.sqrt(ddx * ddx + ddy * ddy), torch.full_like(th, nan))
    G = 1.0 / torch.sqrt(n[None] * J)
    b_.record()
    torch.cuda.synchronize()
    return J, G, a_.elapsed_time(b_)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tables", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", type=int, default=64)
    ap.add_argument("--no-torch", action="store_true", help="time the kernels alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from raytracing_amd import rt_bench as rb
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("eikonal_attr_timing: no GPU; nothing is measured without one")
    P = a.tables
    box = (-2.0, 5.0, -2.5, 1.0)
    grid = (-1.9, 6.8 / (NX - 1), NX, -2.4, 3.3 / (NY - 1), NY)
    F = rb.Field.build("vert_heterogeneous", box, rb.DELTA)
    ys = np.linspace(-2.3, 0.8, P // 2)
    src = np.concatenate([np.stack([np.full(len(ys), 4.85), ys], axis=1), np.stack([np.full(P - len(ys), -1.85), ys[:P - len(ys)]], axis=1)])
    X, Y = np.meshgrid(grid[0] + np.arange(NX) * grid[1], grid[3] + np.arange(NY) * grid[4])
    n = F.n_gradient(X.reshape(-1), Y.reshape(-1))[0].reshape(NY, NX)
    ns = F.n_gradient(src[:, 0], src[:, 1])[0]
    F.close()
    rng = np.random.default_rng(1)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()      # noqa: E731
    d_n, d_src, d_ns = up(n), up(src), up(ns)
    d_dn, d_dns = up(0.1 * n * rng.standard_normal(n.shape)), up(0.1 * ns * rng.standard_normal(P))
    f = rb.eikonal_fill_device(d_n, d_src, grid, None, n_src=d_ns, stats=True)
    assert f["converged"].all()
    tangent = lambda: rb.eikonal_tangent_device(d_n, d_src, grid, f, d_dn, n_src=d_ns, dn_src=d_dns, stats=True)          # noqa: E731
    attr = lambda: rb.eikonal_attributes_device(d_n, d_src, grid, f["T"], f["filled"], n_src=d_ns, stats=True)            # noqa: E731

    def theta0_only():
        """the sweeps alone: the entry with dir, J and G null"""
        import ctypes as C
        from raytracing_amd import _lib
        th = torch.full((P, NY, NX), float("nan"), dtype=torch.float64, device=d_n.device)
        st = _lib.EikonalStats()
        ep = rb.eikonal_params(grid)
        torch.cuda.synchronize()
        _lib.check(_lib.lib().rtmi_eikonal_attributes_dev(C.byref(ep), d_n.data_ptr(), P, d_src.data_ptr(), d_ns.data_ptr(), f["T"].data_ptr(),
                                                          f["filled"].data_ptr(), th.data_ptr(), None, None, None, None, C.byref(st)))
        return st.kernel_ms

    t, at = tangent(), attr()                                                                                            # warm
    theta0_only()
    assert t["converged"].all() and at["converged"].all()
    cap = 16 * (NX + NY)
    if not a.no_torch:
        net = torch_network(torch, d_n, f["T"], f["filled"], d_src, grid)
        one = {k: v[:1] for k, v in net.items()}
        th1, _, _ = torch_theta0(torch, one, d_src[:1], grid, a.check, cap)                                              # warm
        torch_spread(torch, one, th1, d_n, grid)
    tt, ta, ts, jt, jd, iters, diff_th, diff_G = [], [], [], [], [], 0, None, None
    for _ in range(a.reps):                                                                                              # alternating
        t = tangent()
        tt.append(t["stats"]["kernel_ms"])
        at = attr()
        ta.append(at["stats"]["kernel_ms"])
        ts.append(theta0_only())
        if not a.no_torch:
            th, iters, ms = torch_theta0(torch, net, d_src, grid, a.check, cap)
            jt.append(ms)
            J, G, ms = torch_spread(torch, net, th, d_n, grid)
            jd.append(ms)
            fr = net["free"]
            diff_th = float(wrap(torch, th - at["theta0"])[fr].abs().max())
            both = fr & torch.isfinite(G) & torch.isfinite(at["G"])
            diff_G = float(((G - at["G"]).abs() / at["G"].abs().clamp(min=1e-300))[both & (at["G"] > 0)].max())
    nn = NX * NY
    st = at["stats"]
    rounds, rounds_t = int(st["rounds_max"]), int(t["stats"]["rounds_max"])
    sweeps = 4 * rounds
    floors = {"bytes_of_values_weights_and_codes": P * nn * BYTES_PER_NODE * sweeps / HBM * 1e3,
              "diagonals_times_an_l2_round_trip": (NX + NY - 1) * sweeps * L2_ROUND_TRIP / CLOCK * 1e3}
    sa, sk, sy = series(ta), series(ts), series(tt)
    G_host = at["G"].cpu().numpy()
    filled = f["filled"].cpu().numpy() == 1
    out = {"grid": [NX, NY], "tables": P, "reps": a.reps, "path": st["path"], "rounds": at["rounds"].tolist(), "changes": st["changes"],
           "attributes": sa, "theta0_alone": sk, "node_pass_ms": sa["median_ms"] - sk["median_ms"],
           "tangent": sy, "tangent_rounds": rounds_t,
           "ms_per_round": sk["median_ms"] / rounds, "tangent_ms_per_round": sy["median_ms"] / rounds_t,
           "ratio_to_the_tangent_per_round": (sk["median_ms"] / rounds) / (sy["median_ms"] / rounds_t),
           "ratio_of_the_whole_call_to_the_tangent": sa["median_ms"] / sy["median_ms"],
           "ns_per_diagonal": sk["median_ms"] * 1e6 / ((NX + NY - 1) * sweeps), "floor_ms": floors, "binding_floor": max(floors, key=floors.get),
           "G_zero_share": float((G_host[filled] == 0.0).mean()), "G_not_finite_share": float((~np.isfinite(G_host[filled])).mean())}
    if jt:
        sj, sd = series(jt), series(jd)
        total = sj["median_ms"] + sd["median_ms"]
        spread = max(sa["max_ms"] - sa["min_ms"], (sj["max_ms"] - sj["min_ms"]) + (sd["max_ms"] - sd["min_ms"]))
        out.update({"torch_jacobi_theta0": sj, "torch_differences": sd, "jacobi_iterations": iters, "spread_ms": spread,
                    "ratio_of_medians": total / sa["median_ms"], "kernel_is_faster_beyond_the_spread": bool(total - sa["median_ms"] > spread),
                    "largest_theta0_difference_to_jacobi": diff_th, "largest_relative_G_difference_to_torch": diff_G})
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
