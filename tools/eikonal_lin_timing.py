#!/usr/bin/env python3
"""The linearised eikonal fill against two yardsticks, in one process: rtmi_eikonal_tangent_dev and
rtmi_eikonal_adjoint_dev on P = 32 tables of the 737 x 539 grid of tools/eikonal_timing.py (vert_heterogeneous sampled at the
nodes, 32 sources on the lines x = 4.85 and x = -1.85), the tables filled from the source ball alone; warmed, alternating, medians
of --reps device times with min and max.

Yardstick 1 is the forward solve itself: k_eikonal filling the same tables from the ball alone.  A linear sweep walks the same
nx + ny - 1 diagonals with one gather per node, so its time per round is expected near the fill's; that is measured, not assumed.
Yardstick 2 exists without the library: the same gathers as whole-grid Jacobi iterations in plain torch, the coefficients
computed in torch from T as well, every node of every table at once from the previous iterate, run until an iteration changes
nothing (looked at every --check iterations, since the look is a host sync).  Values are compared, not bits, and the largest
difference is printed.

Also printed: the rounds, and the two floors of a sweep kernel -- the bytes of the values, ca, cb, the codes and the constant
term of every sweep at 6 TB/s, and the diagonals of every sweep times a dependent L2 round trip -- and which of them binds.

--linearise factored times the factored update linearised instead: the same 32 tables filled by the
factored scheme from the ball alone, and on them the plain tangent and adjoint (what they were before) against the factored ones,
alternating, medians of --reps device times with min and max; time per round (of the slowest source); and the setup pass on its
own from calls capped at one and at two rounds, setup = 2 t(1) - t(2).  No torch yardstick in this mode.

    python tools/eikonal_lin_timing.py [--tables 32] [--reps 5] [--check 64] [--no-torch] [--linearise plain|factored] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.eikonal_timing import CLOCK, HBM, L2_ROUND_TRIP, NX, NY, series      # noqa: E402

BYTES_PER_NODE = 33                 # the value, ca, cb and the constant term in fp64 and the code, read by every sweep


def torch_network(torch, n, T, filled, src, grid, ball=2.0):
    """the definition's classes and coefficients as tensors [P, ny, nx]: dict of free, ballm, live, ca, cb, cs, east, north"""
    inf = float("inf")
    gx0, gdx, nx, gy0, gdy, ny = grid
    wx, wy = 1.0 / (gdx * gdx), 1.0 / (gdy * gdy)
    A, wxy = wx + wy, wx * wy
    ok = torch.isfinite(n) & (n > 0)
    live = ok[None] & torch.isfinite(T)
    X = gx0 + torch.arange(nx, device=T.device, dtype=torch.float64) * gdx
    Y = gy0 + torch.arange(ny, device=T.device, dtype=torch.float64) * gdy
    dx, dy = X[None, None, :] - src[:, 0, None, None], Y[None, :, None] - src[:, 1, None, None]
    u, v = dx / gdx, dy / gdy
    ballm = live & (filled == 1) & (u * u + v * v <= ball * ball)
    free = live & (filled == 1) & ~ballm
    rp = torch.nn.functional.pad(torch.where(live, T, torch.full_like(T, inf)), (1, 1, 1, 1), value=inf)
    l, r, dn, up = rp[:, 1:-1, :-2], rp[:, 1:-1, 2:], rp[:, :-2, 1:-1], rp[:, 2:, 1:-1]
    east, north = r < l, up < dn
    a, b = torch.where(east, r, l), torch.where(north, up, dn)
    s = torch.where(ok, n, torch.ones_like(n))[None]
    ta, tb = a + gdx * s, b + gdy * s
    e = torch.nan_to_num(a - b, nan=0.0, posinf=0.0, neginf=0.0)
    d = A * (s * s) - wxy * (e * e)
    q = torch.sqrt(torch.clamp(d, min=0.0))
    one_x = (b == inf) | (ta <= b)
    one_y = ~one_x & ((a == inf) | (tb <= a))
    two = ~one_x & ~one_y & (q > 0)
    fall_y = ~one_x & ~one_y & ~two & (tb < ta)
    one_y = one_y | fall_y
    one_x = ~one_y & ~two
    qs = torch.where(two, q, torch.ones_like(q))
    tt = (torch.nan_to_num(a * wx + b * wy, posinf=0.0) + qs) / A
    ca = torch.where(two, (wx * (tt - a)) / qs, one_x.double())
    cb = torch.where(two, (wy * (tt - b)) / qs, one_y.double())
    cs = torch.where(two, s / qs, torch.where(one_x, torch.full_like(q, gdx), torch.full_like(q, gdy)))
    none = (a == inf) & (b == inf)
    ca = torch.where(free & ~none & (a < T), torch.nan_to_num(ca), torch.zeros_like(ca))
    cb = torch.where(free & ~none & (b < T), torch.nan_to_num(cb), torch.zeros_like(cb))
    cs = torch.where(free & ~none, cs, torch.zeros_like(cs))
    cs = torch.where(ballm, 0.5 * torch.sqrt(dx * dx + dy * dy), cs)
    return {"free": free, "ball": ballm, "live": live, "ca": ca, "cb": cb, "cs": cs, "east": east, "north": north}


def jacobi(torch, step, v, check, cap):
    """v <- step(v) until an iteration changes nothing -> (v, iterations, device ms)"""
    a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a_.record()
    it = 0
    while True:
        new = step(v)
        it += 1
        done = it % check == 0 and bool((new == v).all())
        v = new
        if done:
            break
        if it > cap:
            raise SystemExit("eikonal_lin_timing: the Jacobi iteration does not settle")
    b_.record()
    torch.cuda.synchronize()
    return v, it, a_.elapsed_time(b_)


def torch_tangent(torch, net, dn, dns, check, cap):
    pad = torch.nn.functional.pad
    k = net["cs"] * dn[None]
    v0 = torch.where(net["ball"], k + net["cs"] * dns[:, None, None], torch.zeros_like(k))

    def step(v):
        vp = pad(v, (1, 1, 1, 1))
        va = torch.where(net["east"], vp[:, 1:-1, 2:], vp[:, 1:-1, :-2])
        vb = torch.where(net["north"], vp[:, 2:, 1:-1], vp[:, :-2, 1:-1])
        return torch.where(net["free"], (net["ca"] * va + net["cb"] * vb) + k, v0)

    return jacobi(torch, step, v0, check, cap)


def torch_adjoint(torch, net, r, check, cap):
    pad = torch.nn.functional.pad
    cw, ce = net["ca"] * net["east"], net["ca"] * ~net["east"]          # what a node sends east (to its east parent), and west
    cn, cs_ = net["cb"] * net["north"], net["cb"] * ~net["north"]
    r0 = torch.where(net["live"], r, torch.zeros_like(r))

    def step(v):
        w, e, s, n = pad(cw * v, (1, 1, 1, 1)), pad(ce * v, (1, 1, 1, 1)), pad(cn * v, (1, 1, 1, 1)), pad(cs_ * v, (1, 1, 1, 1))
        return torch.where(net["live"], (((r0 + w[:, 1:-1, :-2]) + e[:, 1:-1, 2:]) + s[:, :-2, 1:-1]) + n[:, 2:, 1:-1], r0)

    return jacobi(torch, step, r0, check, cap)


def time_factored(rb, a, grid, d_n, d_src, d_ns, d_dn, d_dns, d_r):
    """the plain and the factored linearisation on the same factored tables -> the dict that is printed"""
    f = rb.eikonal_fill_device(d_n, d_src, grid, None, n_src=d_ns, stats=True, scheme="factored")
    assert f["converged"].all()
    calls = {}
    for lin in ("plain", "factored"):
        calls["tangent", lin] = lambda mr=0, lin=lin: rb.eikonal_tangent_device(d_n, d_src, grid, f, d_dn, n_src=d_ns, dn_src=d_dns, stats=True,
                                                                               max_rounds=mr, linearise=lin)
        calls["adjoint", lin] = lambda mr=0, lin=lin: rb.eikonal_adjoint_device(d_n, d_src, grid, f, d_r, n_src=d_ns, stats=True, max_rounds=mr,
                                                                               linearise=lin)
    res = {k: c() for k, c in calls.items()}                                                                            # warm
    assert all(r["converged"].all() for r in res.values())
    ms = {k: [] for k in calls}
    capped = {(k, mr): [] for k in calls for mr in (1, 2)}
    for _ in range(a.reps):                                                                                             # alternating
        for k, c in calls.items():
            ms[k].append(c()["stats"]["kernel_ms"])
        for (k, mr), v in capped.items():
            v.append(calls[k](mr)["stats"]["kernel_ms"])
    out = {"grid": [NX, NY], "tables": a.tables, "reps": a.reps, "fill_rounds": f["rounds"].tolist(), "fill_ms": f["stats"]["kernel_ms"],
           "maps": []}
    for k in calls:
        sk, rounds = series(ms[k]), int(res[k]["stats"]["rounds_max"])
        t1, t2 = float(np.median(capped[k, 1])), float(np.median(capped[k, 2]))
        case = {"map": k[0], "linearise": k[1], "path": res[k]["stats"]["path"], "rounds": res[k]["rounds"].tolist(), "k_eikonal_lin": sk,
                "ms_per_round": sk["median_ms"] / rounds, "one_round": series(capped[k, 1]), "two_rounds": series(capped[k, 2]),
                "setup_ms": 2 * t1 - t2, "round_ms_from_the_capped_calls": t2 - t1}
        print(json.dumps(case), file=sys.stderr, flush=True)
        out["maps"].append(case)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tables", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", type=int, default=64)
    ap.add_argument("--no-torch", action="store_true", help="time the kernels alone")
    ap.add_argument("--linearise", choices=("plain", "factored"), default="plain", help="factored: DESIGN.md section 40's comparison")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from raytracing_amd import rt_bench as rb
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("eikonal_lin_timing: no GPU; nothing is measured without one")
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
    d_dn, d_dns, d_r = up(0.1 * n * rng.standard_normal(n.shape)), up(0.1 * ns * rng.standard_normal(P)), up(rng.standard_normal((P, NY, NX)))
    if a.linearise == "factored":
        text = json.dumps(time_factored(rb, a, grid, d_n, d_src, d_ns, d_dn, d_dns, d_r), indent=1)
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(text + "\n")
        return
    fill = lambda: rb.eikonal_fill_device(d_n, d_src, grid, None, n_src=d_ns, stats=True)                                  # noqa: E731
    f = fill()                                                                                                           # warm
    assert f["converged"].all()
    tangent = lambda: rb.eikonal_tangent_device(d_n, d_src, grid, f, d_dn, n_src=d_ns, dn_src=d_dns, stats=True)          # noqa: E731
    adjoint = lambda: rb.eikonal_adjoint_device(d_n, d_src, grid, f, d_r, n_src=d_ns, stats=True)                         # noqa: E731
    t, ad = tangent(), adjoint()                                                                                         # warm
    assert t["converged"].all() and ad["converged"].all()
    cap = 16 * (NX + NY)
    if not a.no_torch:
        net = torch_network(torch, d_n, f["T"], f["filled"], d_src, grid)
        one = {k: v[:1] for k, v in net.items()}
        torch_tangent(torch, one, d_dn, d_dns[:1], a.check, cap)                                                         # warm
        torch_adjoint(torch, one, d_r[:1], a.check, cap)
    tf, tt, ta, jt, ja, it_t, it_a, diff_t, diff_a = [], [], [], [], [], 0, 0, None, None
    for _ in range(a.reps):                                                                                              # alternating
        tf.append(fill()["stats"]["kernel_ms"])
        t = tangent()
        tt.append(t["stats"]["kernel_ms"])
        ad = adjoint()
        ta.append(ad["stats"]["kernel_ms"])
        if not a.no_torch:
            v, it_t, ms = torch_tangent(torch, net, d_dn, d_dns, a.check, cap)
            jt.append(ms)
            diff_t = float((v - t["dT"]).abs().max())
            v, it_a, ms = torch_adjoint(torch, net, d_r, a.check, cap)
            ja.append(ms)
            diff_a = float((v - ad["lam"]).abs().max())
    nn = NX * NY
    out = {"grid": [NX, NY], "tables": P, "reps": a.reps, "fill": {"k_eikonal": series(tf), "rounds": f["rounds"].tolist(),
                                                                   "ms_per_round": float(np.median(tf)) / int(f["rounds"].max())}, "maps": []}
    for name, res, tk, tj, iters, diff, big in (("tangent", t, tt, jt, it_t, diff_t, "dT"), ("adjoint", ad, ta, ja, it_a, diff_a, "lam")):
        st = res["stats"]
        rounds = int(st["rounds_max"])
        sweeps = 4 * rounds
        floors = {"bytes_of_values_coefficients_and_codes": P * nn * BYTES_PER_NODE * sweeps / HBM * 1e3,
                  "diagonals_times_an_l2_round_trip": (NX + NY - 1) * sweeps * L2_ROUND_TRIP / CLOCK * 1e3}
        sk = series(tk)
        case = {"map": name, "path": st["path"], "rounds": res["rounds"].tolist(), "changes": st["changes"], "k_eikonal_lin": sk,
                "ms_per_round": sk["median_ms"] / rounds, "ns_per_diagonal": sk["median_ms"] * 1e6 / ((NX + NY - 1) * sweeps),
                "ratio_to_the_fill_per_round": (sk["median_ms"] / rounds) / out["fill"]["ms_per_round"],
                "floor_ms": floors, "binding_floor": max(floors, key=floors.get)}
        if tj:
            sy = series(tj)
            spread = max(sk["max_ms"] - sk["min_ms"], sy["max_ms"] - sy["min_ms"])
            case.update({"torch_jacobi": sy, "jacobi_iterations": iters, "spread_ms": spread,
                         "ratio_of_medians": sy["median_ms"] / sk["median_ms"],
                         "kernel_is_faster_beyond_the_spread": bool(sy["median_ms"] - sk["median_ms"] > spread),
                         "largest_difference_to_jacobi": diff, "largest_value": float(res[big].abs().max())})
        print(json.dumps(case), file=sys.stderr, flush=True)
        out["maps"].append(case)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
