"""The eikonal continuation of a traveltime table restated (rtmi_eikonal_fill, include/rtmi.h; raytracing_amd/csrc/rt_eikonal.h;
DESIGN.md section 34) in plain Python floats: every product, sum, quotient and sqrt below is one rounded fp64 operation, and the
loops are the serial sweeps that define the result.  Arrays go in and out as numpy, the arithmetic runs on Python lists."""
import math

import numpy as np

INF = math.inf
NAN = math.nan
DEFAULT_ROUNDS = 64
FROZEN, FREE, BALL = 0, 1, 2


def fmin(x, y):
    return y if y < x else x


def obstacle(s):
    return not (math.isfinite(s) and s > 0.0)


def init(grid, i, j, s, tin, xs, ys, n_src, ball):
    """(state, starting value) of node (i, j) with slowness s and input tin"""
    gx0, gdx, _, gy0, gdy, _ = grid
    if obstacle(s):
        return FROZEN, INF
    if math.isfinite(tin):
        return FROZEN, tin
    if not (ball >= 0.0) or obstacle(n_src):
        return FREE, INF
    X = gx0 + float(i) * gdx
    Y = gy0 + float(j) * gdy
    dx = X - xs
    dy = Y - ys
    u = dx / gdx
    v = dy / gdy
    if not (u * u + v * v <= ball * ball):
        return FREE, INF
    return BALL, (0.5 * (n_src + s)) * math.sqrt(dx * dx + dy * dy)


def update(gdx, gdy, a, b, s):
    """The candidate value of a free node from a = min of its x neighbours and b = min of its y neighbours; +inf: no change"""
    if a == INF and b == INF:
        return INF
    ta = a + gdx * s
    tb = b + gdy * s
    if b == INF or ta <= b:
        return ta
    if a == INF or tb <= a:
        return tb
    wx = 1.0 / (gdx * gdx)
    wy = 1.0 / (gdy * gdy)
    A = wx + wy
    B = a * wx + b * wy
    e = a - b
    d = A * (s * s) - (wx * wy) * (e * e)
    if d < 0.0:
        return fmin(ta, tb)
    return (B + math.sqrt(d)) / A


def solve_one(grid, n, xs, ys, n_src, T=None, ball=2.0, max_rounds=0):
    """One source: (T [ny, nx], rounds, clean, filled [ny, nx] uint8, changes).  T=None: every input NaN."""
    gx0, gdx, nx, gy0, gdy, ny = grid
    gx0, gdx, gy0, gdy, nx, ny = float(gx0), float(gdx), float(gy0), float(gdy), int(nx), int(ny)
    g = (gx0, gdx, nx, gy0, gdy, ny)
    nl = [float(v) for v in np.asarray(n, dtype=np.float64).reshape(-1)]
    tin = [NAN] * (nx * ny) if T is None else [float(v) for v in np.asarray(T, dtype=np.float64).reshape(-1)]
    assert len(nl) == len(tin) == nx * ny
    xs, ys, n_src, ball = float(xs), float(ys), float(n_src), float(ball)
    st, w = [0] * (nx * ny), [INF] * (nx * ny)
    seeds = free_now = 0
    for j in range(ny):
        for i in range(nx):
            x = j * nx + i
            st[x], w[x] = init(g, i, j, nl[x], tin[x], xs, ys, n_src, ball)
            if st[x] == FREE:
                free_now += 1
            elif w[x] < INF:
                seeds += 1
    cap = max_rounds if max_rounds > 0 else DEFAULT_ROUNDS
    rounds, clean, changes = 0, 1, 0
    # what the update derives from the spacings alone, once: the same operations on the same operands, hence the same bits
    wx = 1.0 / (gdx * gdx)
    wy = 1.0 / (gdy * gdy)
    A = wx + wy
    wxy = wx * wy
    sqrt = math.sqrt
    if free_now > 0 and seeds > 0:
        free = [[x for x in range(j * nx, (j + 1) * nx) if st[x] == FREE] for j in range(ny)]
        while rounds < cap:
            rounds += 1
            changed = 0
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
                        a = r if r < l else l
                        b = up if up < dn else dn
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
                            w[x] = t
                            changed += 1
            changes += changed
            clean = int(changed == 0)
            if clean:
                break
    out = np.array(tin, dtype=np.float64)
    filled = np.zeros(nx * ny, dtype=np.uint8)
    for x in range(nx * ny):
        if st[x] != FROZEN:
            got = w[x] < INF
            out[x] = w[x] if got else NAN
            filled[x] = 1 if got else 0
    return out.reshape(ny, nx), rounds, clean, filled.reshape(ny, nx), changes


def solve(grid, n, sources, n_src, T=None, ball=2.0, max_rounds=0):
    """Every source of sources [S, 2]: dict of T [S, ny, nx], rounds [S], converged [S], filled [S, ny, nx], changes"""
    src = np.asarray(sources, dtype=np.float64).reshape(-1, 2)
    ns = np.asarray(n_src, dtype=np.float64).reshape(-1)
    S, ny, nx = len(src), int(grid[5]), int(grid[2])
    out = {"T": np.empty((S, ny, nx)), "rounds": np.zeros(S, dtype=np.int32), "converged": np.zeros(S, dtype=np.int32),
           "filled": np.zeros((S, ny, nx), dtype=np.uint8), "changes": 0}
    for s in range(S):
        t, r, c, f, ch = solve_one(grid, n, src[s, 0], src[s, 1], ns[s], None if T is None else np.asarray(T)[s], ball, max_rounds)
        out["T"][s], out["rounds"][s], out["converged"][s], out["filled"][s] = t, r, c, f
        out["changes"] += ch
    return out


def same_bits(a, b):
    """doubles equal bit for bit, NaN payloads and the sign of zero included"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---------------------------------------------------------------------------------------------- media and truths for the tests
def gradient_truth(X, Y, xs, ys, v0=18.0, gy=2.0):
    """The traveltime from (xs, ys) in v = v0 + gy y (n = 1 / v): (1 / |gy|) arccosh(1 + gy^2 r^2 / (2 v_s v_r))"""
    vs, vr = v0 + gy * ys, v0 + gy * np.asarray(Y, dtype=np.float64)
    r2 = (np.asarray(X, dtype=np.float64) - xs) ** 2 + (np.asarray(Y, dtype=np.float64) - ys) ** 2
    return np.arccosh(1.0 + gy * gy * r2 / (2.0 * vs * vr)) / abs(gy)


def nodes(grid):
    gx0, gdx, nx, gy0, gdy, ny = grid
    return np.meshgrid(float(gx0) + np.arange(int(nx)) * float(gdx), float(gy0) + np.arange(int(ny)) * float(gdy))


def winding_corridor(nx=31, ny=27, wall=1000.0, flip=True):
    """A corridor of slowness 1, one node wide, between walls of slowness `wall`, one node thick, that spirals inwards from a
    corner of the grid: the first arrival from its outer end follows it, and each turn costs the sweeps a round.  flip: the
    spiral turns from +x to -y (against the order of the sweeps), else from +x to +y.  Returns (n [ny, nx], (ix, iy) of the
    corridor's outer end)."""
    n = np.full((ny, nx), float(wall))
    dirs = ((1, 0), (0, 1), (-1, 0), (0, -1))
    inside = lambda i, j: 1 <= i <= nx - 2 and 1 <= j <= ny - 2
    open_ = lambda i, j: inside(i, j) and n[j, i] == 1.0
    i, j, d = 1, 1, 0
    n[j, i] = 1.0
    while True:
        for turn in (0, 1):
            di, dj = dirs[(d + turn) % 4]
            if inside(i + di, j + dj) and not open_(i + di, j + dj) and not open_(i + 2 * di, j + 2 * dj):
                d = (d + turn) % 4
                break
        else:
            break
        i, j = i + di, j + dj
        n[j, i] = 1.0
    return (n[::-1].copy(), (1, ny - 2)) if flip else (n, (1, 1))
