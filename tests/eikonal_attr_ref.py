"""Launch angle, direction and spreading at eikonal-filled nodes restated (rtmi_eikonal_attributes, include/rtmi.h;
raytracing_amd/csrc/rt_eikonal_attr.h) in plain Python floats over tests/eikonal_lin_ref.Net: every
product, sum, quotient and sqrt below is one rounded fp64 operation, and math.atan2 is the libm the library's host side calls.
Arrays go in and out as numpy, the arithmetic runs on Python lists.  order= picks the schedule that finds the launch angle's
fixed point: "sweeps" (the definition, which also defines rounds), "other" (the adjoint's sweep orders) and "sorted" (one pass
over the free nodes sorted by T)."""
import math

import numpy as np

import eikonal_lin_ref as L
import eikonal_ref as R

INF, NAN = math.inf, math.nan
PI, TWO_PI = math.pi, 2.0 * math.pi


def div(a, b):
    """a / b as IEEE gives it where b is zero"""
    if b == 0.0:
        if a == 0.0 or a != a:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def wrap(d):
    if d > PI:
        return d - TWO_PI
    if d <= -PI:
        return d + TWO_PI
    return d


def weight(par, ca, cb):
    both = L.XPARENT | L.YPARENT
    return div(cb, ca + cb) if par & both == both else 0.0


def combine(has_a, ta, has_b, tb, w):
    ua = has_a and math.isfinite(ta)
    ub = has_b and math.isfinite(tb)
    if ua and ub:
        r = ta + w * wrap(tb - ta)
        return r if r == r else NAN
    if ua:
        return ta
    if ub:
        return tb
    return NAN


def ball_dir(dx, dy, r):
    return (dx / r, dy / r) if r > 0.0 else (0.0, 0.0)


def free_dir(gdx, gdy, par, t, a, b):
    gx = gy = 0.0
    if par & L.XPARENT:
        d = t - a
        gx = (-d if par & L.XEAST else d) / gdx
    if par & L.YPARENT:
        d = t - b
        gy = (-d if par & L.YNORTH else d) / gdy
    m = math.sqrt(gx * gx + gy * gy)
    return (gx / m, gy / m) if m > 0.0 else (NAN, NAN)


def diff(use_lo, lo, t, use_hi, hi, h):
    if use_lo and use_hi:
        return wrap(hi - lo) / (2.0 * h)
    if use_hi:
        return wrap(hi - t) / h
    if use_lo:
        return wrap(t - lo) / h
    return 0.0


def spread(ddx, ddy):
    return div(1.0, math.sqrt(ddx * ddx + ddy * ddy))


def amp(s, J):
    return div(1.0, math.sqrt(s * J))


def solve_one(grid, n, xs, ys, n_src, T, filled, theta0=None, px=None, py=None, J=None, G=None, ball=2.0, max_rounds=0,
              order="sweeps", net=None):
    """One source: dict of theta0, px, py, J, G [ny, nx], rounds, clean, changes and the network.  Absent inputs are all NaN."""
    gx0, gdx, nx, gy0, gdy, ny = grid
    gx0, gdx, gy0, gdy, nx, ny = float(gx0), float(gdx), float(gy0), float(gdy), int(nx), int(ny)
    nn = nx * ny
    xs, ys = float(xs), float(ys)
    net = net or L.Net(grid, n, xs, ys, n_src, T, filled, ball)
    nl = [float(v) for v in np.asarray(n, dtype=np.float64).reshape(-1)]
    tl = net.T
    as_list = lambda a: [NAN] * nn if a is None else [float(v) for v in np.asarray(a, dtype=np.float64).reshape(-1)]   # noqa: E731
    th, pxl, pyl, Jl, Gl = as_list(theta0), as_list(px), as_list(py), as_list(J), as_list(G)
    cls, par = net.cls, net.par
    w = [weight(par[x], net.ca[x], net.cb[x]) if cls[x] == L.FREE else 0.0 for x in range(nn)]
    geo = {}
    for x in range(nn):
        if cls[x] == L.BALL:
            i, j = x % nx, x // nx
            X = gx0 + float(i) * gdx
            Y = gy0 + float(j) * gdy
            dx = X - xs
            dy = Y - ys
            geo[x] = (dx, dy, math.sqrt(dx * dx + dy * dy))
            th[x] = math.atan2(dy, dx)
        elif cls[x] == L.FREE:
            th[x] = NAN

    def gather(x):
        p = par[x]
        ha, hb = bool(p & L.XPARENT), bool(p & L.YPARENT)
        ta = th[x + 1 if p & L.XEAST else x - 1] if ha else 0.0
        tb = th[x + nx if p & L.YNORTH else x - nx] if hb else 0.0
        return combine(ha, ta, hb, tb, w[x])

    rounds, clean, changes = net.run(gather, th, net.free, False, order, max_rounds)
    alive = [cls[x] != L.DEAD for x in range(nn)]
    for x in range(nn):
        if cls[x] == L.BALL:
            dx, dy, r = geo[x]
            pxl[x], pyl[x] = ball_dir(dx, dy, r)
            Jl[x] = r
        elif cls[x] == L.FREE:
            i, j = x % nx, x // nx
            p = par[x]
            a = tl[x + 1 if p & L.XEAST else x - 1] if p & L.XPARENT else 0.0
            b = tl[x + nx if p & L.YNORTH else x - nx] if p & L.YPARENT else 0.0
            pxl[x], pyl[x] = free_dir(gdx, gdy, p, tl[x], a, b)
            t = th[x]
            if math.isfinite(t):
                uw = i > 0 and alive[x - 1] and math.isfinite(th[x - 1])
                ue = i + 1 < nx and alive[x + 1] and math.isfinite(th[x + 1])
                us = j > 0 and alive[x - nx] and math.isfinite(th[x - nx])
                un = j + 1 < ny and alive[x + nx] and math.isfinite(th[x + nx])
                ddx = diff(uw, th[x - 1] if uw else 0.0, t, ue, th[x + 1] if ue else 0.0, gdx)
                ddy = diff(us, th[x - nx] if us else 0.0, t, un, th[x + nx] if un else 0.0, gdy)
                Jl[x] = spread(ddx, ddy)
            else:
                Jl[x] = NAN
        else:
            continue
        Gl[x] = amp(nl[x], Jl[x]) if Jl[x] == Jl[x] else NAN
    arr = lambda a: np.array(a, dtype=np.float64).reshape(ny, nx)      # noqa: E731
    return {"theta0": arr(th), "px": arr(pxl), "py": arr(pyl), "J": arr(Jl), "G": arr(Gl), "rounds": rounds, "clean": clean,
            "changes": changes, "net": net}


def solve(grid, n, sources, n_src, fill, theta0=None, px=None, py=None, J=None, G=None, ball=2.0, max_rounds=0, order="sweeps",
          nets=None):
    """Every source: dict of theta0, px, py, J, G [S, ny, nx], rounds, converged [S], changes, nets"""
    src = np.asarray(sources, dtype=np.float64).reshape(-1, 2)
    ns = np.asarray(n_src, dtype=np.float64).reshape(-1)
    S = len(src)
    keys = ("theta0", "px", "py", "J", "G")
    ins = dict(zip(keys, (theta0, px, py, J, G)))
    out = {k: [] for k in keys}
    out.update(rounds=np.zeros(S, dtype=np.int32), converged=np.zeros(S, dtype=np.int32), changes=0, nets=[])
    for s in range(S):
        one = solve_one(grid, n, src[s, 0], src[s, 1], ns[s], fill["T"][s], fill["filled"][s],
                        **{k: None if v is None else np.asarray(v)[s] for k, v in ins.items()}, ball=ball, max_rounds=max_rounds,
                        order=order, net=None if nets is None else nets[s])
        for k in keys:
            out[k].append(one[k])
        out["rounds"][s], out["converged"][s] = one["rounds"], one["clean"]
        out["changes"] += one["changes"]
        out["nets"].append(one["net"])
    for k in keys:
        out[k] = np.stack(out[k]) if S else np.zeros((0, int(grid[5]), int(grid[2])))
    return out


KEYS = ("theta0", "px", "py", "J", "G")


def same(got, want, keys=KEYS):
    """every array bit for bit with NaN compared by place, and rounds and converged; returns the first that differs or None"""
    for k in keys:
        if not L.same_but_nan(got[k], want[k]):
            return k
    for k in ("rounds", "converged"):
        if not np.array_equal(np.asarray(got[k]), np.asarray(want[k])):
            return k
    return None


# ------------------------------------------------------------------------------------------------ closed forms for the tests
def gradient_theta0(X, Y, xs, ys, v0=18.0, gy=2.0):
    """The launch angle at (xs, ys) of the ray to (X, Y) in v = v0 + gy y: the tangent at the source of the circle through both
    points whose centre lies on the line v = 0.  The sign of X - xs picks the half-plane the ray leaves into."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    y0 = -v0 / gy                                   # v = 0
    dx = X - xs
    with np.errstate(divide="ignore", invalid="ignore"):
        xc = xs + (dx * dx + (Y - y0) ** 2 - (ys - y0) ** 2) / (2.0 * dx)
    # the radius vector from the centre to the source is (xs - xc, ys - y0); the tangent is perpendicular, pointing towards X
    tx, ty = (ys - y0) * np.sign(dx), (xc - xs) * np.sign(dx)
    th = np.arctan2(ty, tx)
    vertical = dx == 0.0
    return np.where(vertical, np.where(Y >= ys, 0.5 * np.pi, -0.5 * np.pi), th)


def gradient_J(X, Y, xs, ys, v0=18.0, gy=2.0):
    """|dx/dtheta0| at constant T in v = v0 + gy y: v_r sinh(g T) / g"""
    T = R.gradient_truth(X, Y, xs, ys, v0, gy)
    return (v0 + gy * np.asarray(Y, dtype=np.float64)) * np.sinh(abs(gy) * T) / abs(gy)


def seeded_disc(shape=(71, 57), holes=((3.0, -1.0, 0.49),)):
    """disc_case on a grid of `shape` nodes over the same extent, with the closed-form theta0 at every node: (grid, n, src, ns,
    T, theta0 [S, ny, nx] closed form, J closed form).  holes: (x, y, radius squared) of each disc the table leaves out"""
    nx, ny = shape
    grid = (-2.0, 7.0 / (nx - 1), nx, -2.5, 3.5 / (ny - 1), ny)
    X, Y = R.nodes(grid)
    n = 1.0 / (18.0 + 2.0 * Y)
    src = np.array(L.GRADIENT_SOURCES)
    ns = 1.0 / (18.0 + 2.0 * src[:, 1])
    out = np.zeros(X.shape, dtype=bool)
    for hx, hy, r2 in holes:
        out |= (X - hx) ** 2 + (Y - hy) ** 2 <= r2
    T = np.stack([np.where(out, np.nan, R.gradient_truth(X, Y, xs, ys)) for xs, ys in src])
    th = np.stack([gradient_theta0(X, Y, xs, ys) for xs, ys in src])
    Jc = np.stack([gradient_J(X, Y, xs, ys) for xs, ys in src])
    return grid, n, src, ns, T, th, Jc
