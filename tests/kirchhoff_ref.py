"""numpy restatement of the Kirchhoff operator pair (include/rtmi.h, rtmi_kirchhoff_*): migrate as the
loop over traces k = 0 .. N-1 the header defines (every operation a separate fp64 operation in its order, so the device's
image is reproduced bit for bit), model as the same weights in a scipy CSR matrix; the standard case of the tests on the
closed forms of v = 18 + 2 y (traveltimes: ttgrid_ref.vert_T; directions: arcs of circles centred on y = -9)."""
import numpy as np

import ttgrid_ref as G

TWO_PI = 2.0 * np.pi


def terms(T, s, r, wk, nt, dt, t0=0.0, amp=None, theta=None, nbin=0, dopen=None):
    """One trace against every node: (x, b, j, a, c) of the contributing pairs; x the flat node index, c None when no factor is
    present (factors that are absent are left out)."""
    P = T.shape[0]
    Tf = T.reshape(P, -1)
    inv_dt = 1.0 / dt
    with np.errstate(invalid="ignore", over="ignore"):
        tau = Tf[s] + Tf[r]
        f = (tau - t0) * inv_dt
        jf = np.floor(f)
        a = f - jf
        ok = np.isfinite(Tf[s]) & np.isfinite(Tf[r]) & (jf >= 0) & (jf <= nt - 2)
        c = None
        if amp is not None:
            Af = amp.reshape(P, -1)
            ok &= np.isfinite(Af[s]) & np.isfinite(Af[r])
            c = Af[s] * Af[r] if wk is None else (wk * Af[s]) * Af[r]
        elif wk is not None:
            c = np.full(Tf.shape[1], float(wk))
        b = np.zeros(Tf.shape[1], dtype=np.int64)
        if nbin > 0:
            Hf = theta.reshape(P, -1)
            d = Hf[s] - Hf[r]
            h = 0.5 * np.abs(d - TWO_PI * np.rint(d / TWO_PI))
            hb = np.floor(h / dopen)
            ok &= np.isfinite(Hf[s]) & np.isfinite(Hf[r]) & (hb < nbin)
            b = np.where(ok, hb, 0).astype(np.int64)
    x = np.nonzero(ok)[0]
    return x, b[x], jf[x].astype(np.int64), a[x], None if c is None else c[x]


def migrate(T, isrc, irec, data, dt, t0=0.0, amp=None, theta=None, w=None, nbin=0, dopen=None):
    """-> (image [max(nbin, 1), ny, nx], contributing pairs): the header's loop, traces in the caller's order"""
    P, ny, nx = T.shape
    N, nt = data.shape
    nn = ny * nx
    img = np.zeros(max(nbin, 1) * nn)
    count = 0
    for k in range(N):
        x, b, j, a, c = terms(T, isrc[k], irec[k], None if w is None else w[k], nt, dt, t0, amp, theta, nbin, dopen)
        d0, d1 = data[k, j], data[k, j + 1]
        v = d0 + a * (d1 - d0)
        if c is not None:
            v = c * v
        img[b * nn + x] += v                 # one trace meets a (bin, node) at most once
        count += len(x)
    return img.reshape(max(nbin, 1), ny, nx), count


def matrix(T, isrc, irec, nt, dt, t0=0.0, amp=None, theta=None, w=None, nbin=0, dopen=None):
    """L as a CSR matrix [N nt, max(nbin, 1) ny nx]: rows k nt + j and k nt + j + 1 get c (1 - a) and c a"""
    from scipy.sparse import csr_matrix
    P, ny, nx = T.shape
    nn = ny * nx
    N = len(isrc)
    rows, cols, vals = [], [], []
    for k in range(N):
        x, b, j, a, c = terms(T, isrc[k], irec[k], None if w is None else w[k], nt, dt, t0, amp, theta, nbin, dopen)
        c = 1.0 if c is None else c
        rows += [k * nt + j, k * nt + j + 1]
        cols += [b * nn + x, b * nn + x]
        vals += [c * (1.0 - a), c * a]
    return csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N * nt, max(nbin, 1) * nn))


# ------------------------------------------------------------------------------------------------ the standard case
POS_Y = -2.4
POS_X = np.linspace(-1.5, 4.5, 48) + 1e-3          # the 1e-3 keeps x != xs at every node
GRID = (-1.0, 0.025, 201, -2.0, 0.025, 101)
DT, T0, NT = 0.001, 0.0, 1024
SCATTERER = (120, 60)                              # (ix, iy)
NBIN, DOPEN = 6, np.pi / 12
FREQ = 60.0


def grid_xy(grid=GRID):
    gx0, gdx, nx, gy0, gdy, ny = grid
    return np.meshgrid(gx0 + np.arange(nx) * gdx, gy0 + np.arange(ny) * gdy)


def geometry(pos=48, every=4):
    """sources every 4th position, receivers all: shot-ordered (isrc, irec)"""
    src = np.arange(0, pos, every)
    isrc = np.repeat(src, pos).astype(np.int32)
    irec = np.tile(np.arange(pos), len(src)).astype(np.int32)
    return isrc, irec


def closed_T(pos_x=POS_X, pos_y=POS_Y, grid=GRID):
    X, Y = grid_xy(grid)
    return np.stack([G.vert_T(xs, pos_y, X, Y) for xs in pos_x])


def closed_theta(pos_x=POS_X, pos_y=POS_Y, grid=GRID):
    """The ray direction at each node: rays of v = 18 + 2 y are arcs of circles centred on (xc, -9)"""
    X, Y = grid_xy(grid)
    out = []
    for xs in pos_x:
        xc = ((X ** 2 - xs ** 2) + (Y + 9) ** 2 - (pos_y + 9) ** 2) / (2 * (X - xs))
        sg = np.sign(xc - xs)
        out.append(np.arctan2(-sg * (X - xc), sg * (Y + 9)))
    return np.stack(out)


def ricker(t, f=FREQ):
    u = (np.pi * f * t) ** 2
    return (1.0 - 2.0 * u) * np.exp(-u)


def scatterer_data(isrc, irec, node=SCATTERER, pos_x=POS_X, pos_y=POS_Y, grid=GRID, nt=NT, dt=DT, t0=T0):
    """a 60 Hz Ricker centred on the closed-form T_s + T_r of a scatterer at the node"""
    gx0, gdx, _, gy0, gdy, _ = grid
    x, y = gx0 + node[0] * gdx, gy0 + node[1] * gdy
    Tp = G.vert_T(pos_x, pos_y, x, y)
    t = t0 + np.arange(nt) * dt
    return ricker(t[None, :] - (Tp[isrc] + Tp[irec])[:, None])


def half_opening(theta, isrc, irec, node=SCATTERER):
    d = theta[isrc, node[1], node[0]] - theta[irec, node[1], node[0]]
    return 0.5 * np.abs(d - TWO_PI * np.rint(d / TWO_PI))


def lsm_model(grid=GRID):
    """The least-squares migration model: two point scatterers and a dipping segment"""
    _, _, nx, _, _, ny = grid
    m = np.zeros((ny, nx))
    m[60, 120] = 1.0
    m[40, 60] = -1.0
    ix = np.arange(80, 161)
    m[70 - (ix - 80) // 4, ix] = 0.5
    return m


def with_holes(a, rng, share=0.05):
    """NaN in a share of the table nodes: how traveltime_table marks nodes a fan does not cover"""
    a = a.copy()
    a[rng.random(a.shape) < share] = np.nan
    return a
