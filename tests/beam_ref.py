"""numpy restatement of rtmi_gaussian_beams (include/rtmi.h; raytracing_amd/csrc/beams.hip): the rows' values of the prep, the
ownership, q_max and cutoff tests, the interpolation and the sum, in the device's operation order.  Test infrastructure.

Q1 P1 Q2 P2 and n after every row come from rtmi_paraxial's propagator (tests/paraxial_ref.py) on scipy's fits, where the device
evaluates the same splines as cell polynomials (< 1e-15 of each quantity's scale apart).  cos and sin of the rows are np.cos /
np.sin (glibc's, which the device reproduces); arctan2, exp, cos and sin of the phases are numpy's where the device uses ocml's,
so the sums agree to rounding, not bit for bit.  The device only tests the pairs of the tiles a step was binned into; binning is
conservative, so the restatement tests every pair."""
import numpy as np

from crossing_ref import _basis, _herm
from paraxial_ref import kappa, kdk

CUTOFF = 18.0
WIDTH_CELLS = 64.0
COS_TURN = 0.5403023058681398      # cos(1): a step that turns more than 1 rad owns no node


def wrap(d):
    return d - 6.283185307179586 * np.rint(d / 6.283185307179586)


def nodes(grid):
    """X, Y [ny, nx] of grid = (gx0, gdx, nx, gy0, gdy, ny), computed as the device does"""
    gx0, gdx, nx, gy0, gdy, ny = grid
    X = gx0 + np.arange(int(nx)).astype(np.float64) * gdx
    Y = gy0 + np.arange(int(ny)).astype(np.float64) * gdy
    return np.broadcast_to(X[None, :], (int(ny), int(nx))), np.broadcast_to(Y[:, None], (int(ny), int(nx)))


def tube_rows(s_ray, last, field):
    """Q1 P1 Q2 P2 n after every row 0 .. min(last, rows - 1) of every ray (rtmi_paraxial's walk) -> [rows, 5, R]"""
    s_ray = np.asarray(s_ray)
    rows, _, R = s_ray.shape
    last = np.minimum(np.asarray(last, dtype=np.int64), rows - 1)
    x, y, th = (s_ray[:, q, :].astype(np.float64) for q in (0, 1, 5))
    c, s = np.cos(th), np.sin(th)
    live = np.arange(rows)[:, None] <= last[None, :]
    f = [np.ones((rows, R))] + [np.zeros((rows, R)) for _ in range(6)]
    vals = field(x[live], y[live])
    for q in range(7):
        f[q][live] = vals[q]
    K = kappa(f, c, s)
    w = 1.0 / f[0]
    out = np.full((rows, 5, R), np.nan)
    t = [np.ones(R), np.zeros(R), np.zeros(R), np.ones(R)]
    out[0, :4] = np.array(t)
    out[0, 4] = f[0][0]
    for i in range(1, int(last.max()) + 1):
        act = live[i]
        dx, dy = x[i] - x[i - 1], y[i] - y[i - 1]
        ln = np.sqrt(dx * dx + dy * dy)
        nt = kdk(t, ln, K[i - 1], K[i], 0.5 * (w[i - 1] + w[i]))
        t = [np.where(act, a, b) for a, b in zip(nt, t)]
        for q in range(4):
            out[i, q] = np.where(act, t[q], np.nan)
        out[i, 4] = np.where(act, f[0][i], np.nan)
    return out


def weights(theta0, fan_size, edge_taper=0.0):
    """the trapezoid weights in theta0 of every fan, times the cosine edge taper"""
    th = np.asarray(theta0, dtype=np.float64).reshape(-1, int(fan_size))
    nxt = np.concatenate([th[:, 1:], th[:, -1:]], axis=1)
    prv = np.concatenate([th[:, :1], th[:, :-1]], axis=1)
    w = 0.5 * np.abs(nxt - prv)
    if edge_taper > 0:
        d = np.minimum(np.abs(th - th[:, :1]), np.abs(th - th[:, -1:]))
        w = np.where(d < edge_taper, w * (0.5 * (1.0 - np.cos(np.pi * d / edge_taper))), w)
    return w.ravel()


def ray_rows(s_ray, tube, o, nr, w_o, eps):
    """k_prep for ray o: dict of its rows' values"""
    col = lambda q: np.asarray(s_ray[:nr, q, o], dtype=np.float64)
    x, y, T, th = col(0), col(1), col(4), col(5)
    q1, p1, q2, p2, n = (tube[:nr, q, o] for q in range(5))
    eq1, ep1 = eps * q1, eps * p1
    qq = q2 * q2 + eq1 * eq1
    re = (p2 * q2 + ep1 * eq1) / qq
    im = (eps * (p2 * q1 - p1 * q2)) / qq
    a = np.arctan2(-eq1, q2)
    phi = np.cumsum(np.concatenate([[-0.5 * np.pi], wrap(a[1:] - a[:-1])]))
    W = w_o * np.sqrt(eps * tube[0, 4, o]) / (4.0 * np.pi)
    amp = W / np.sqrt(n * np.sqrt(qq))
    return dict(x=x, y=y, c=np.cos(th), s=np.sin(th), T=T, n=n, re=re, im=im, phi=phi, amp=amp, qq=qq)


NEAR = 1e-12      # relative distance of a deciding quantity from its threshold below which a pair counts as `near`


def gaussian_beams(s_ray, last, field, theta0, fan_size, grid, omegas, eps, cutoff=None, max_width=None, edge_taper=0.0,
                   tube=None, counts=None):
    """s_ray [rows, 6, R], last [R] (each ray's last written row; rows past the record are cut), field: a SplineField (or any
    callable of its signature), theta0 [R] the launch angles.  -> u [S, nw, ny, nx] complex128 as rtmi_gaussian_beams.
    counts: a dict to fill with what rtmi_beam_stats counts, from every (step, node) pair: segments (the sum over rays of
    rows - 1), capped (steps that pass the turn test and whose uncapped q_max exceeds max_width), owned and inside (pairs before
    and after the q_max and cutoff tests at the lowest omega), inside_per_omega, and near: the owned pairs one of whose deciding
    quantities lies within NEAR (relative) of its threshold -- d_{i-1} or d_i against 0 relative to |X - x| + |Y - y|, q^2
    against q_max^2, omega_min g against the cutoff -- the pairs a last-bit difference in the rows' values could flip."""
    s_ray = np.asarray(s_ray)
    rows, _, R = s_ray.shape
    last = np.minimum(np.asarray(last, dtype=np.int64), rows - 1)
    if tube is None:
        tube = tube_rows(s_ray, last, field)
    gx0, gdx, nx, gy0, gdy, ny = grid
    cutoff = float(cutoff) if cutoff else CUTOFF
    maxw = float(max_width) if max_width else WIDTH_CELLS * max(gdx, gdy)
    om = np.atleast_1d(np.asarray(omegas, dtype=np.float64))
    omin = om.min()
    w = weights(theta0, fan_size, edge_taper)
    M = int(fan_size)
    S = R // M
    X, Y = (a.ravel() for a in nodes(grid))
    ar = np.zeros((S, len(om), X.size))
    ai = np.zeros((S, len(om), X.size))
    cn = dict(segments=int(last.sum()), capped=0, owned=0, inside=0, inside_per_omega=[0] * len(om), near=0)
    for o in range(R):
        s = o // M
        v = ray_rows(s_ray, tube, o, int(last[o]) + 1, w[o], eps)
        if len(v["x"]) < 2:
            continue
        d = (X[None, :] - v["x"][:, None]) * v["c"][:, None] + (Y[None, :] - v["y"][:, None]) * v["s"][:, None]
        turn_ok = (v["c"][:-1] * v["c"][1:] + v["s"][:-1] * v["s"][1:]) >= COS_TURN
        own = (d[:-1] >= 0.0) & (d[1:] < 0.0) & turn_ok[:, None]
        qm_step = np.sqrt(2.0 * cutoff * np.maximum(v["qq"][:-1], v["qq"][1:]) / (omin * eps))
        cn["capped"] += int((turn_ok & (qm_step > maxw)).sum())
        i, k = np.nonzero(own)                     # row-major: by step, then node -- per node the device's (m, i) order
        if i.size == 0:
            continue
        A = {key: val[i] for key, val in v.items()}
        B = {key: val[i + 1] for key, val in v.items()}
        Xk, Yk = X[k], Y[k]
        da = (Xk - A["x"]) * A["c"] + (Yk - A["y"]) * A["s"]
        db = (Xk - B["x"]) * B["c"] + (Yk - B["y"]) * B["s"]
        lam = da / (da - db)
        px = A["x"] + lam * (B["x"] - A["x"])
        py = A["y"] + lam * (B["y"] - A["y"])
        tcx = A["c"] + lam * (B["c"] - A["c"])
        tcy = A["s"] + lam * (B["s"] - A["s"])
        qn = (Xk - px) * (-tcy) + (Yk - py) * tcx
        q2 = (qn * qn) / (tcx * tcx + tcy * tcy)
        qq = np.maximum(A["qq"], B["qq"])
        qm = np.sqrt(2.0 * cutoff * qq / (omin * eps))
        qm = np.where(qm > maxw, maxw, qm)
        im = A["im"] + lam * (B["im"] - A["im"])
        g = 0.5 * im * q2
        keep = (q2 <= qm * qm) & ~(omin * g > cutoff)
        cn["owned"] += int(i.size)
        cn["inside"] += int(keep.sum())
        cn["near"] += int(((np.abs(da) <= NEAR * (np.abs(Xk - A["x"]) + np.abs(Yk - A["y"]))) |
                           (np.abs(db) <= NEAR * (np.abs(Xk - B["x"]) + np.abs(Yk - B["y"]))) |
                           (np.abs(q2 - qm * qm) <= NEAR * (qm * qm)) | (np.abs(omin * g - cutoff) <= NEAR * cutoff)).sum())
        if not keep.any():
            continue
        sel = lambda a: a[keep]
        lam, q2, g, k = sel(lam), sel(q2), sel(g), sel(k)
        A = {key: sel(val) for key, val in A.items()}
        B = {key: sel(val) for key, val in B.items()}
        re = A["re"] + lam * (B["re"] - A["re"])
        ph = A["phi"] + lam * (B["phi"] - A["phi"])
        am = A["amp"] + lam * (B["amp"] - A["amp"])
        dx, dy = B["x"] - A["x"], B["y"] - A["y"]
        L = np.sqrt(dx * dx + dy * dy)
        T = _herm(_basis(lam), A["T"], L * A["n"], B["T"], L * B["n"])
        h = T + 0.5 * re * q2
        hp = 0.5 * ph
        for q, wq in enumerate(om):
            wg = wq * g
            ok = wg <= cutoff
            cn["inside_per_omega"][q] += int(ok.sum())
            amp = am[ok] * np.exp(-wg[ok])
            arg = wq * h[ok] - hp[ok]
            np.add.at(ar[s, q], k[ok], amp * np.cos(arg))
            np.add.at(ai[s, q], k[ok], amp * np.sin(arg))
    c = 0.7071067811865476
    u = c * (ar - ai) + 1j * (c * (ar + ai))
    if counts is not None:
        counts.update(cn)
    return u.reshape(S, len(om), int(ny), int(nx))


def ray_theory(T, G, kmah, omega):
    """the ray-theory Green's function of rtmi_paraxial: G / sqrt(8 pi omega) exp(i (omega T - kmah pi/2 + pi/4))"""
    return G / np.sqrt(8.0 * np.pi * omega) * np.exp(1j * (omega * T - kmah * np.pi / 2 + np.pi / 4))
