#!/usr/bin/env python3
"""Eikonal continuation of traveltime tables against the same update in plain torch, in one process:
rtmi_eikonal_fill_dev completing P = 32 tables on the 737 x 539 grid of section 29's timing case, once seeded by traced fans
(vert_heterogeneous, op6, 32 stations on the lines x = 4.85 and x = -1.85, five cells inside the grid, half-plane fans of --rays rays towards its middle) and once from the source
ball alone (no table), warmed, alternating, medians of --reps device times with min and max.

The yardstick exists without the library: the same Godunov update as a whole-grid Jacobi iteration in broadcast tensor ops on the
device, every free node of every table at once from the previous iterate, run until an iteration changes nothing (looked at every
--check iterations, since the look is a host sync); timed with torch events around the whole loop.  Jacobi and the sweeps reach
the same fixed point by different orders of rounding: values are compared, not bits, and the largest difference is printed.  The
rule is DESIGN.md section 24's: the kernel is accepted where its series lies below torch's by more than the spread of the two.

Also printed: the rounds, the share of nodes that were free, and the two floors of the kernel -- the bytes of T, n and the states
of every sweep at 6 TB/s, and the diagonals of every sweep times a dependent L2 round trip, since a diagonal reads what the one
before it wrote -- and which of them binds.

--scheme factored times the source-factored scheme against the plain one instead of the plain one against
torch: the two kernels alternate in the same process on the same two cases, and what is printed is each one's series, rounds and
time per round, the ratio of the rounds and of a round's cost, the largest difference between the two tables, and each table's
largest error against the closed form of the medium, (1 / 2) arccosh(1 + 2 r^2 / (v_s v_r)), as a fraction of its largest T.

    python tools/eikonal_timing.py [--tables 32] [--rays 1024] [--reps 5] [--check 64] [--no-torch] [--scheme plain|factored]
                                   [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 6.0e12                        # bytes per second
CLOCK = 2.4e9
L2_ROUND_TRIP = 225                 # cycles of an L2-hit load on an idle chip: the least a diagonal can wait for the one before it
BYTES_PER_NODE = 17                 # T and n in fp64 and the state, read by every sweep
NX, NY = 737, 539


def series(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}


def torch_jacobi(torch, n, T0, free, gdx, gdy, check):
    """the yardstick: T0 [P, ny, nx] with +inf at the free nodes -> (T, iterations, device ms)"""
    inf = float("inf")
    wx, wy = 1.0 / (gdx * gdx), 1.0 / (gdy * gdy)
    A, wxy = wx + wy, wx * wy
    hx, hy, nn2 = gdx * n, gdy * n, A * (n * n)
    T = T0.clone()
    a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a_.record()
    it = 0
    while True:
        Tp = torch.nn.functional.pad(T, (1, 1, 1, 1), value=inf)
        a = torch.minimum(Tp[:, 1:-1, :-2], Tp[:, 1:-1, 2:])
        b = torch.minimum(Tp[:, :-2, 1:-1], Tp[:, 2:, 1:-1])
        ta, tb = a + hx, b + hy
        e = torch.nan_to_num(a - b, nan=0.0, posinf=0.0, neginf=0.0)
        d = nn2 - wxy * (e * e)
        two = (torch.nan_to_num(a * wx + b * wy, posinf=0.0) + torch.sqrt(torch.clamp(d, min=0.0))) / A
        t = torch.where((b == inf) | (ta <= b), ta, torch.where((a == inf) | (tb <= a), tb, torch.where(d < 0, torch.minimum(ta, tb), two)))
        new = torch.where(free, torch.minimum(T, t), T)
        it += 1
        done = it % check == 0 and bool((new == T).all())             # a look is a host sync: one every `check` iterations
        T = new
        if done:
            break
        if it > 16 * (NX + NY):
            raise SystemExit("eikonal_timing: the Jacobi iteration does not settle")
    b_.record()
    torch.cuda.synchronize()
    return T, it, a_.elapsed_time(b_)


def factored_against_plain(torch, rb, name, dn, dsrc, dns, grid, start, X, Y, reps):
    """one case of --scheme factored: both kernels warmed, alternating, their series and what the factoring buys and costs"""
    run = lambda scheme: rb.eikonal_fill_device(dn, dsrc, grid, start.clone(), n_src=dns, stats=True, scheme=scheme)       # noqa: E731
    res = {k: run(k) for k in ("plain", "factored")}                                                                    # warm
    ms = {"plain": [], "factored": []}
    for _ in range(reps):                                                                                               # alternating
        for k in ms:
            res[k] = run(k)
            ms[k].append(res[k]["stats"]["kernel_ms"])
    Xd, Yd = torch.from_numpy(X).cuda()[None], torch.from_numpy(Y).cuda()[None]
    xs, ys = dsrc[:, 0, None, None], dsrc[:, 1, None, None]
    truth = 0.5 * torch.acosh(1.0 + 4.0 * ((Xd - xs) ** 2 + (Yd - ys) ** 2) / (2.0 * (18.0 + 2.0 * ys) * (18.0 + 2.0 * Yd)))
    # The closed form is the time along the circular arc through both points whose centre lies on y = -9; where that arc rises
    # above the grid's top row between its ends, the solve, which knows the grid alone, has no such path and the closed form is
    # not its truth: those nodes are left out of the second error figure.
    yc, top = -9.0, float(Y.max())
    xc = ((Xd * Xd - xs * xs) + (Yd - yc) ** 2 - (ys - yc) ** 2) / (2.0 * (Xd - xs))          # not finite straight above the source
    leaves = ((xc - xs) * (xc - Xd) < 0.0) & (yc + torch.sqrt((xs - xc) ** 2 + (ys - yc) ** 2) > top)
    case = {"case": name, "path": res["plain"]["stats"]["path"], "largest_T_s": float(truth.max()),
            "share_of_nodes_whose_ray_leaves_the_grid": float(leaves.double().mean())}
    for k in ms:
        st, sk = res[k]["stats"], series(ms[k])
        rounds = int(st["rounds_max"])
        filled = res[k]["filled"] != 0
        err = float(((res[k]["T"] - truth).abs() * filled).max() / truth.max()) if bool(filled.any()) else 0.0
        inside = filled & ~leaves
        err_in = float(((res[k]["T"] - truth).abs() * inside).max() / truth.max()) if bool(inside.any()) else 0.0
        case[k] = {"k_eikonal": sk, "rounds": sorted(set(res[k]["rounds"].tolist())), "converged": bool(res[k]["converged"].all()),
                   "changes": st["changes"], "unreached": st["unreached"], "ms_per_round": sk["median_ms"] / max(rounds, 1),
                   "ns_per_diagonal": sk["median_ms"] * 1e6 / ((NX + NY - 1) * 4 * max(rounds, 1)),
                   "error_at_filled_nodes_of_largest_T": err, "error_where_the_ray_stays_in_the_grid": err_in}
    both = torch.isfinite(res["plain"]["T"]) & torch.isfinite(res["factored"]["T"])
    case["largest_difference_s"] = float((res["plain"]["T"] - res["factored"]["T"])[both].abs().max())
    case["ratio_of_medians"] = case["factored"]["k_eikonal"]["median_ms"] / case["plain"]["k_eikonal"]["median_ms"]
    case["ratio_of_rounds"] = max(case["factored"]["rounds"]) / max(max(case["plain"]["rounds"]), 1)
    case["ratio_of_a_round"] = case["factored"]["ms_per_round"] / case["plain"]["ms_per_round"]
    return case


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tables", type=int, default=32)
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", type=int, default=64)
    ap.add_argument("--no-torch", action="store_true", help="time the kernel alone")
    ap.add_argument("--scheme", choices=("plain", "factored"), default="plain", help="factored: time it against the plain scheme")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from raytracing_amd import rt_bench as rb
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("eikonal_timing: no GPU; nothing is measured without one")
    P = a.tables
    box = (-2.0, 5.0, -2.5, 1.0)
    grid = (-1.9, 6.8 / (NX - 1), NX, -2.4, 3.3 / (NY - 1), NY)
    F = rb.Field.build("vert_heterogeneous", box, rb.DELTA)
    ys = np.linspace(-2.3, 0.8, P // 2)
    right, left = np.stack([np.full(len(ys), 4.85), ys], axis=1), np.stack([np.full(P - len(ys), -1.85), ys[:P - len(ys)]], axis=1)
    src = np.concatenate([right, left])
    kw = dict(step=rb.DELTA_S, max_size=int(np.ceil(80 / rb.DELTA_S) + 1), box=box)
    tabs = [rb.traveltime_table(rb.op6, F, right, grid, thetas=np.linspace(np.pi / 2 + 0.02, 3 * np.pi / 2 - 0.02, a.rays), **kw),
            rb.traveltime_table(rb.op6, F, left, grid, thetas=np.linspace(-np.pi / 2 + 0.02, np.pi / 2 - 0.02, a.rays), **kw)]
    traced = np.concatenate([t["T"] for t in tabs])
    X, Y = np.meshgrid(grid[0] + np.arange(NX) * grid[1], grid[3] + np.arange(NY) * grid[4])
    n = F.n_gradient(X.reshape(-1), Y.reshape(-1))[0].reshape(NY, NX)
    ns = F.n_gradient(src[:, 0], src[:, 1])[0]
    F.close()
    dn, dsrc, dns = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (n, src, ns))
    nn = NX * NY
    out = {"grid": [NX, NY], "tables": P, "rays": a.rays, "reps": a.reps, "cases": []}
    for name, seed in (("traced fans", traced), ("ball alone", None)):
        start = torch.full((P, NY, NX), float("nan"), dtype=torch.float64, device="cuda") if seed is None else torch.from_numpy(seed).cuda()
        if a.scheme == "factored":
            case = factored_against_plain(torch, rb, name, dn, dsrc, dns, grid, start, X, Y, a.reps)
            print(json.dumps(case), file=sys.stderr, flush=True)
            out["cases"].append(case)
            continue
        kernel = lambda: rb.eikonal_fill_device(dn, dsrc, grid, start.clone(), n_src=dns, stats=True)            # noqa: E731
        r = kernel()                                                                                              # warm
        # the yardstick starts from the kernel's own frozen values, the ball's included: only the iteration differs
        u = (torch.from_numpy(X).cuda()[None] - dsrc[:, 0, None, None]) / grid[1]
        v = (torch.from_numpy(Y).cuda()[None] - dsrc[:, 1, None, None]) / grid[4]
        free = ~torch.isfinite(start) & ~(u * u + v * v <= 4.0)
        T0 = torch.where(free, torch.full_like(start, float("inf")), r["T"])
        del u, v
        tk, tt, iters, diff = [], [], 0, None
        if not a.no_torch:
            torch_jacobi(torch, dn, T0[:1], free[:1], grid[1], grid[4], a.check)                                  # warm
        for _ in range(a.reps):                                                                                   # alternating
            r = kernel()
            tk.append(r["stats"]["kernel_ms"])
            if not a.no_torch:
                Tj, iters, ms = torch_jacobi(torch, dn, T0, free, grid[1], grid[4], a.check)
                tt.append(ms)
                both = torch.isfinite(Tj) & torch.isfinite(r["T"])
                diff = float((Tj - r["T"])[both].abs().max()) if bool(both.any()) else 0.0
        st = r["stats"]
        rounds = int(st["rounds_max"])
        sweeps = 4 * rounds
        floors = {"bytes_of_T_n_and_states": P * nn * BYTES_PER_NODE * sweeps / HBM * 1e3,
                  "diagonals_times_an_l2_round_trip": (NX + NY - 1) * sweeps * L2_ROUND_TRIP / CLOCK * 1e3}
        sk = series(tk)
        case = {"case": name, "path": st["path"], "rounds": r["rounds"].tolist(), "free_share": st["free_nodes"] / (P * nn),
                "unreached": st["unreached"], "changes": st["changes"], "k_eikonal": sk,
                "ns_per_diagonal": sk["median_ms"] * 1e6 / ((NX + NY - 1) * sweeps) if sweeps else None,
                "floor_ms": floors, "binding_floor": max(floors, key=floors.get)}
        if tt:
            sy = series(tt)
            spread = max(sk["max_ms"] - sk["min_ms"], sy["max_ms"] - sy["min_ms"])
            case.update({"torch_jacobi": sy, "jacobi_iterations": iters, "spread_ms": spread,
                         "ratio_of_medians": sy["median_ms"] / sk["median_ms"],
                         "kernel_is_faster_beyond_the_spread": bool(sy["median_ms"] - sk["median_ms"] > spread),
                         "largest_difference_to_jacobi_s": diff, "largest_T_s": float(torch.nan_to_num(r["T"], nan=0.0).max())})
        print(json.dumps(case), file=sys.stderr, flush=True)
        out["cases"].append(case)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
