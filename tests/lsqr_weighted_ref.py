"""Restatement of the weighted, masked and warm-started solvers (include/rtmi.h, rtmi_lsqr_options) on top
of kirchhoff_lsqr_ref.lsqr_loop, and of rtmi_kirchhoff_illumination on top of the pair loops of kirchhoff_ref / kirchhoff_multi_ref.
numpy forms every product as a temporary, so every product and every add is rounded on its own, as the header states it.  Test
infrastructure."""
import numpy as np

import kirchhoff_lsqr_ref as R
import kirchhoff_multi_ref as KM


def _flat(a):
    return None if a is None else np.asarray(a, dtype=np.float64).reshape(-1)


def _leading(f, t):
    """t with its leading len(f) values multiplied by f: the rows after them carry no factor (an absent factor is left out)"""
    if f is None:
        return t
    t = t.copy()
    t[:f.size] = f * t[:f.size]
    return t


def lsqr_weighted(matvec, rmatvec, b, iter_lim, wr=None, dc=None, x0=None, ndata=None, **kw):
    """min |W A D y - W (b - A x0)|^2 + damp^2 |y|^2 by lsqr_loop, x = x0 + D y.  matvec / rmatvec are the operator without
    options; b may be longer than its ndata leading data rows, which wr covers (a regulariser's rows: no weight, and A x0 is not
    subtracted from them -- their right-hand side stays as given).  -> lsqr_loop's dict, with y beside x.  With no option: lsqr_loop itself."""
    wr, dc, x0 = _flat(wr), _flat(dc), _flat(x0)
    if wr is None and dc is None and x0 is None:
        return R.lsqr_loop(matvec, rmatvec, b, iter_lim, **kw)
    r = np.asarray(b, dtype=np.float64).reshape(-1).copy()
    ndata = (r.size if wr is None else wr.size) if ndata is None else ndata
    if x0 is not None:
        t = np.asarray(matvec(x0), dtype=np.float64).reshape(-1)
        r[:ndata] = r[:ndata] - t[:ndata]
    r = _leading(wr, r)

    def fwd(v):
        s = v if dc is None else dc * v
        return _leading(wr, np.asarray(matvec(s), dtype=np.float64).reshape(-1))

    def bwd(u):
        t = np.asarray(rmatvec(_leading(wr, np.asarray(u, dtype=np.float64).reshape(-1))), dtype=np.float64).reshape(-1)
        return t if dc is None else dc * t

    out = R.lsqr_loop(fwd, bwd, r, iter_lim, **kw)
    y = out["x"]
    x = y if dc is None else dc * y
    if x0 is not None:
        x = x0 + x
    out["y"], out["x"] = y, x
    return out


def illumination(T, isrc, irec, nt, dt, t0=0.0, amp=None, theta=None, kmah=None, w=None, nbin=0, dopen=None, pt=None):
    """-> (illum [max(nbin, 1), ny, nx], contributing pairs) for tables [P, K, ny, nx]: per (b, x) the sum, from +0.0 and in
    migrate's order k, ks, kr, of fl(fl(c c) fl(fl(fl(1 - a) fl(1 - a)) + fl(a a))) over migrate's contributing pairs (with pt:
    those whose two pt are finite as well).  A c that no factor makes is 1."""
    P, Karr, ny, nx = T.shape
    nn = ny * nx
    ill = np.zeros(max(nbin, 1) * nn)
    count = 0
    for k in range(len(isrc)):
        for ks in range(Karr):
            for kr in range(Karr):
                x, b, j, a, c, q = KM.pair_terms(T, isrc[k], ks, irec[k], kr, None if w is None else w[k], nt, dt, t0, amp, theta,
                                                 kmah, nbin, dopen)
                if pt is not None:
                    ok = np.isfinite(pt[isrc[k], ks].reshape(-1)[x]) & np.isfinite(pt[irec[k], kr].reshape(-1)[x])
                    x, b, a = x[ok], b[ok], a[ok]
                    c = None if c is None else c[ok]
                om = 1.0 - a
                g = om * om + a * a
                cc = np.ones(len(x)) if c is None else c * c
                ill[b * nn + x] += cc * g                     # one pair of arrivals meets a (bin, node) at most once
                count += len(x)
    return ill.reshape(max(nbin, 1), ny, nx), count


# ------------------------------------------------------------------------------------------------ the tiny case
# 30 nodes, so that every unit model can be imaged: one arrival per node, a NaN patch in one table
P, NY, NX, N, NT, DT = 4, 5, 6, 9, 32, 0.001


def tiny_case(amp=False, nbin=0):
    rng = np.random.default_rng(23)
    T = 0.002 + 0.55 * NT * DT * rng.random((P, NY, NX))
    T[2, 1:3, 2:5] = np.nan                                           # a patch the fan does not cover
    th = rng.uniform(-np.pi, np.pi, (P, NY, NX))
    isrc = np.sort(rng.integers(0, P, N)).astype(np.int32)
    irec = rng.integers(0, P, N).astype(np.int32)
    kw = dict(amp=0.5 + rng.random((P, NY, NX)) if amp else None, theta=th if nbin else None, w=rng.standard_normal(N) if amp else None,
              nbin=nbin, dopen=0.45 * np.pi / nbin if nbin else None)
    return T, isrc, irec, kw
