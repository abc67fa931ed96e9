"""The source-factored scheme of the eikonal fill restated (rtmi_eikonal_params.scheme = RTMI_EIKONAL_FACTORED, include/rtmi.h;
raytracing_amd/csrc/rt_eikonal.h) in plain Python floats, on top of eikonal_ref, which holds everything the
scheme leaves as it is: the states, the ball, the update, the sweep orders, the round rule, `filled` and unreached -> NaN.  Every
product, sum, quotient and sqrt below is one rounded fp64 operation.

Additive factoring: T = T0 + u with T0 = n_src r, the traveltime of the source's own slowness.  Differencing u upwind is the plain
update on shifted neighbour readings: the parent's value plus the truncation error of differencing T0 across that edge.  For node
(i, j) of a source, in eikonal_ref.init's expressions,
    X = gx0 + float(i) gdx;  dx = X - xs;  Y = gy0 + float(j) gdy;  dy = Y - ys;  rr = sqrt(dx dx + dy dy);  T0 = n_src rr
Factoring is left out for a source whose n_src is an obstacle's (not finite or <= 0) and at a node with rr == 0: the plain update.
Otherwise the update of a free node reads l, r, dn, up as the plain one does and then
    x-parent east iff r < l;  a_raw = that reading
      a = a_raw == +inf ? +inf : (a_raw + (T0[x] - T0[parent])) +- px;  px = gdx (n_src (dx / rr));  + for east, - for west
    y-parent north iff up < dn;  b_raw = that reading
      b = b_raw == +inf ? +inf : (b_raw + (T0[x] - T0[parent])) +- py;  py = gdy (n_src (dy / rr));  + for north, - for south
    t = update(a, b, s), unchanged;  T[x] = t iff t < T[x]
The side is chosen on the raw readings.  T0 is a function of the node alone, so a table of it and a fresh evaluation have the
same bits; solve_one keeps tables, readings() evaluates afresh."""
import math

import numpy as np

import eikonal_ref as R

PLAIN, FACTORED = 0, 1
INF = math.inf


def t0(grid, i, j, xs, ys, n_src):
    """(T0, dx, dy, rr) of node (i, j)"""
    gx0, gdx, _, gy0, gdy, _ = grid
    X = gx0 + float(i) * gdx
    Y = gy0 + float(j) * gdy
    dx = X - xs
    dy = Y - ys
    rr = math.sqrt(dx * dx + dy * dy)
    return n_src * rr, dx, dy, rr


def readings(grid, i, j, xs, ys, n_src, l, r, dn, up):
    """(a, b), what the unchanged update takes at node (i, j) from its four neighbour readings"""
    gdx, gdy = grid[1], grid[4]
    east, north = r < l, up < dn
    a = r if east else l
    b = up if north else dn
    if R.obstacle(n_src):
        return a, b
    T0x, dx, dy, rr = t0(grid, i, j, xs, ys, n_src)
    if rr == 0.0:
        return a, b
    if a != INF:
        px = gdx * (n_src * (dx / rr))
        a = a + (T0x - t0(grid, i + 1 if east else i - 1, j, xs, ys, n_src)[0])
        a = a + px if east else a - px
    if b != INF:
        py = gdy * (n_src * (dy / rr))
        b = b + (T0x - t0(grid, i, j + 1 if north else j - 1, xs, ys, n_src)[0])
        b = b + py if north else b - py
    return a, b


def update(grid, i, j, xs, ys, n_src, l, r, dn, up, s):
    """The candidate value of free node (i, j) with slowness s; +inf: no change"""
    a, b = readings(grid, i, j, xs, ys, n_src, l, r, dn, up)
    return R.update(grid[1], grid[4], a, b, s)


def solve_one(grid, n, xs, ys, n_src, T=None, ball=2.0, max_rounds=0, scheme=FACTORED, history=None):
    """One source, as eikonal_ref.solve_one: (T [ny, nx], rounds, clean, filled [ny, nx] uint8, changes).  history: a list that
    gets the largest decrease of any node in each round."""
    if scheme not in (PLAIN, FACTORED):
        raise ValueError("scheme")
    if scheme == PLAIN or R.obstacle(float(n_src)):
        return R.solve_one(grid, n, xs, ys, n_src, T=T, ball=ball, max_rounds=max_rounds)
    gx0, gdx, nx, gy0, gdy, ny = grid
    gx0, gdx, gy0, gdy, nx, ny = float(gx0), float(gdx), float(gy0), float(gdy), int(nx), int(ny)
    g = (gx0, gdx, nx, gy0, gdy, ny)
    nl = [float(v) for v in np.asarray(n, dtype=np.float64).reshape(-1)]
    tin = [R.NAN] * (nx * ny) if T is None else [float(v) for v in np.asarray(T, dtype=np.float64).reshape(-1)]
    assert len(nl) == len(tin) == nx * ny
    xs, ys, n_src, ball = float(xs), float(ys), float(n_src), float(ball)
    st, w = [0] * (nx * ny), [INF] * (nx * ny)
    T0, px, py, plain = [0.0] * (nx * ny), [0.0] * (nx * ny), [0.0] * (nx * ny), [False] * (nx * ny)
    seeds = free_now = 0
    for j in range(ny):
        for i in range(nx):
            x = j * nx + i
            st[x], w[x] = R.init(g, i, j, nl[x], tin[x], xs, ys, n_src, ball)
            if st[x] == R.FREE:
                free_now += 1
            elif w[x] < INF:
                seeds += 1
            T0[x], dx, dy, rr = t0(g, i, j, xs, ys, n_src)
            plain[x] = rr == 0.0
            if not plain[x]:
                px[x] = gdx * (n_src * (dx / rr))
                py[x] = gdy * (n_src * (dy / rr))
    cap = max_rounds if max_rounds > 0 else R.DEFAULT_ROUNDS
    rounds, clean, changes = 0, 1, 0
    wx = 1.0 / (gdx * gdx)
    wy = 1.0 / (gdy * gdy)
    A = wx + wy
    wxy = wx * wy
    sqrt = math.sqrt
    if free_now > 0 and seeds > 0:
        free = [[x for x in range(j * nx, (j + 1) * nx) if st[x] == R.FREE] for j in range(ny)]
        while rounds < cap:
            rounds += 1
            changed = 0
            drop = 0.0
            for k in range(4):
                xup, yup = k in (0, 3), k < 2
                for j in (range(ny) if yup else range(ny - 1, -1, -1)):
                    row = free[j]
                    lo, hi = j * nx, (j + 1) * nx - 1
                    for x in (row if xup else reversed(row)):
                        l = w[x - 1] if x > lo else INF
                        r = w[x + 1] if x < hi else INF
                        dn = w[x - nx] if j > 0 else INF
                        up = w[x + nx] if j + 1 < ny else INF
                        if plain[x]:
                            a = r if r < l else l
                            b = up if up < dn else dn
                        else:
                            if r < l:
                                a = r if r == INF else (r + (T0[x] - T0[x + 1])) + px[x]
                            else:
                                a = l if l == INF else (l + (T0[x] - T0[x - 1])) - px[x]
                            if up < dn:
                                b = up if up == INF else (up + (T0[x] - T0[x + nx])) + py[x]
                            else:
                                b = dn if dn == INF else (dn + (T0[x] - T0[x - nx])) - py[x]
                        if a == INF and b == INF:
                            continue
                        s = nl[x]
                        ta = a + gdx * s
                        tb = b + gdy * s
                        if b == INF or ta <= b:
                            t = ta
                        elif a == INF or tb <= a:
                            t = tb
                        else:
                            B = a * wx + b * wy
                            e = a - b
                            d = A * (s * s) - wxy * (e * e)
                            t = (tb if tb < ta else ta) if d < 0.0 else (B + sqrt(d)) / A
                        if t < w[x]:
                            if w[x] < INF and w[x] - t > drop:
                                drop = w[x] - t
                            w[x] = t
                            changed += 1
            changes += changed
            clean = int(changed == 0)
            if history is not None:
                history.append(drop)
            if clean:
                break
    out = np.array(tin, dtype=np.float64)
    filled = np.zeros(nx * ny, dtype=np.uint8)
    for x in range(nx * ny):
        if st[x] != R.FROZEN:
            got = w[x] < INF
            out[x] = w[x] if got else R.NAN
            filled[x] = 1 if got else 0
    return out.reshape(ny, nx), rounds, clean, filled.reshape(ny, nx), changes


def solve(grid, n, sources, n_src, T=None, ball=2.0, max_rounds=0, scheme=FACTORED):
    """Every source of sources [S, 2], as eikonal_ref.solve"""
    src = np.asarray(sources, dtype=np.float64).reshape(-1, 2)
    ns = np.asarray(n_src, dtype=np.float64).reshape(-1)
    S, ny, nx = len(src), int(grid[5]), int(grid[2])
    out = {"T": np.empty((S, ny, nx)), "rounds": np.zeros(S, dtype=np.int32), "converged": np.zeros(S, dtype=np.int32),
           "filled": np.zeros((S, ny, nx), dtype=np.uint8), "changes": 0}
    for s in range(S):
        t, r, c, f, ch = solve_one(grid, n, src[s, 0], src[s, 1], ns[s], None if T is None else np.asarray(T)[s], ball, max_rounds,
                                   scheme)
        out["T"][s], out["rounds"][s], out["converged"][s], out["filled"][s] = t, r, c, f
        out["changes"] += ch
    return out


# ---------------------------------------------------------------------------------------------- the cases of the truth table
GRIDS = {71: (-2.0, 7.0 / 70, 71, -2.5, 3.5 / 56, 57), 141: (-2.0, 7.0 / 140, 141, -2.5, 3.5 / 112, 113)}
SOURCES = ((-1.97, -2.03), (1.513, -0.77))


def gradient_medium(grid, v0=18.0, gy=2.0):
    """(X, Y, n) with n = 1 / (v0 + gy y) at the nodes"""
    X, Y = R.nodes(grid)
    return X, Y, 1.0 / (v0 + gy * Y)
