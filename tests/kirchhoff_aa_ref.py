"""numpy restatement of the Kirchhoff pair anti-aliased by operator slope (include/rtmi.h, rtmi_kirchhoff_create_aa /
rtmi_kirchhoff_aa_filter).  tri is the triangle filter F_k in the header's order of operations; level the
level rule; pair_terms is kirchhoff_multi_ref.pair_terms with the finite test on pt and the level of each contributing pair;
migrate is the loop that defines the device's bits; matrix is L as CSR over [2][N][nt] x [nb][ny][nx], the F_k included.
Test infrastructure; also the closed-form launch angles of v = 18 + 2 y and the tests' small random case."""
import numpy as np

import kirchhoff_multi_ref as KM
import kirchhoff_ref as K1

HW8 = (0, 1, 2, 4, 8, 16, 32, 64)


def tri(d, k):
    """F_k along the last axis: (sum over i = -k .. k, 0 <= j + i < nt, of (k + 1 - |i|) * d[j+i]) * inv_k, i ascending from a
    sum of 0.0, every product and add a separate fp64 operation"""
    d = np.asarray(d, dtype=np.float64)
    nt = d.shape[-1]
    n = float(k + 1)
    inv = 1.0 / (n * n)
    out = np.zeros_like(d)
    for i in range(-k, k + 1):
        lo, hi = max(0, -i), min(nt, nt - i)              # the samples j with 0 <= j + i < nt
        if lo < hi:
            out[..., lo:hi] = out[..., lo:hi] + float(k + 1 - abs(i)) * d[..., lo + i:hi + i]
    return out * inv


def tri_matrix(nt, k):
    """F_k as a dense [nt, nt] matrix: column i is the filter of the i-th unit vector"""
    return tri(np.eye(nt), k).T


def level(ps, pr, hw, dt, asrc=0.0, arec=0.0, amid=0.0):
    """The level rule: the smallest index with sl <= hw[l], else the last one"""
    inv_dt = 1.0 / dt
    with np.errstate(invalid="ignore", over="ignore"):
        q1 = np.abs(ps) * asrc
        q2 = np.abs(pr) * arec
        q3 = np.abs(ps + pr) * amid
        sl = np.fmax(np.fmax(q1, q2), q3) * inv_dt
        lev = np.zeros(np.shape(sl), dtype=np.int64)
        for h in hw[:-1]:
            lev += sl > float(h)
    return lev


def pair_terms(T, pt, aa, s, ks, r, kr, wk, nt, dt, t0=0.0, **kw):
    """kirchhoff_multi_ref.pair_terms of the pairs whose two pt are finite, and their levels: (x, b, j, a, c, q, l)"""
    x, b, j, a, c, q = KM.pair_terms(T, s, ks, r, kr, wk, nt, dt, t0, **kw)
    ps, pr = pt[s, ks].reshape(-1)[x], pt[r, kr].reshape(-1)[x]
    ok = np.isfinite(ps) & np.isfinite(pr)
    x, b, j, a, q, ps, pr = x[ok], b[ok], j[ok], a[ok], q[ok], ps[ok], pr[ok]
    c = None if c is None else c[ok]
    return x, b, j, a, c, q, level(ps, pr, aa["hw"], dt, aa.get("asrc", 0.0), aa.get("arec", 0.0), aa.get("amid", 0.0))


def bank(d, hw):
    """[nlev, ...]: level 0 the traces as given"""
    return np.stack([np.asarray(d, dtype=np.float64)] + [tri(d, k) for k in hw[1:]])


def migrate(T, pt, aa, isrc, irec, d0, d1, dt, t0=0.0, amp=None, theta=None, kmah=None, w=None, nbin=0, dopen=None):
    """-> (image [max(nbin, 1), ny, nx], contributing pairs): the header's loop, k ascending, then ks, then kr, each pair on its
    level's copy of its channel"""
    P, Karr, ny, nx = T.shape
    N, nt = d0.shape
    nn = ny * nx
    img = np.zeros(max(nbin, 1) * nn)
    B = [bank(d0, aa["hw"]), None if kmah is None else bank(d1, aa["hw"])]
    count = 0
    for k in range(N):
        for ks in range(Karr):
            for kr in range(Karr):
                x, b, j, a, c, q, lev = pair_terms(T, pt, aa, isrc[k], ks, irec[k], kr, None if w is None else w[k], nt, dt, t0,
                                                   amp=amp, theta=theta, kmah=kmah, nbin=nbin, dopen=dopen)
                if kmah is None:
                    e0, e1 = B[0][lev, k, j], B[0][lev, k, j + 1]
                else:
                    odd = KM.CHANNEL[q] == 1
                    e0 = np.where(odd, B[1][lev, k, j], B[0][lev, k, j])
                    e1 = np.where(odd, B[1][lev, k, j + 1], B[0][lev, k, j + 1])
                v = e0 + a * (e1 - e0)
                if c is not None:
                    v = c * v
                img[b * nn + x] += KM.SIGN[q] * v             # one pair of arrivals meets a (bin, node) at most once
                count += len(x)
    return img.reshape(max(nbin, 1), ny, nx), count


def matrix(T, pt, aa, isrc, irec, nt, dt, t0=0.0, amp=None, theta=None, kmah=None, w=None, nbin=0, dopen=None):
    """L as a CSR matrix [2 N nt, max(nbin, 1) ny nx]: the sum over the levels of (F_hw[l] on every trace) times the spread matrix of
    the level's pairs, whose row (ch N + k) nt + j gets sg c (1 - a), the next one sg c a"""
    from scipy.sparse import csr_matrix, identity, kron
    P, Karr, ny, nx = T.shape
    nn = ny * nx
    N = len(isrc)
    hw = aa["hw"]
    shape = (2 * N * nt, max(nbin, 1) * nn)
    rows, cols, vals = ([[] for _ in hw] for _ in range(3))
    for k in range(N):
        for ks in range(Karr):
            for kr in range(Karr):
                x, b, j, a, c, q, lev = pair_terms(T, pt, aa, isrc[k], ks, irec[k], kr, None if w is None else w[k], nt, dt, t0,
                                                   amp=amp, theta=theta, kmah=kmah, nbin=nbin, dopen=dopen)
                c = KM.SIGN[q] * (1.0 if c is None else c)
                row = (KM.CHANNEL[q] * N + k) * nt + j
                for l in range(len(hw)):
                    at = lev == l
                    rows[l] += [row[at], row[at] + 1]
                    cols[l] += [(b * nn + x)[at]] * 2
                    vals[l] += [(c * (1.0 - a))[at], (c * a)[at]]
    L = csr_matrix(shape)
    for l, k in enumerate(hw):
        S = csr_matrix((np.concatenate(vals[l]), (np.concatenate(rows[l]), np.concatenate(cols[l]))), shape=shape)
        L = L + (S if l == 0 else kron(identity(2 * N), csr_matrix(tri_matrix(nt, k)), format="csr") @ S)
    return L.tocsr()


# ------------------------------------------------------------------------------------------------ closed forms of v = 18 + 2 y
def closed_theta0(pos_x=K1.POS_X, pos_y=K1.POS_Y, grid=K1.GRID):
    """The launch angle at each position of the ray to each node: rays are arcs of circles centred on (xc, -9)
    (kirchhoff_ref.closed_theta is the same arc's direction at the node)"""
    X, Y = K1.grid_xy(grid)
    out = []
    for xs in pos_x:
        xc = ((X ** 2 - xs ** 2) + (Y + 9) ** 2 - (pos_y + 9) ** 2) / (2 * (X - xs))
        sg = np.sign(xc - xs)
        out.append(np.arctan2(-sg * (xs - xc), sg * (pos_y + 9)))
    return np.stack(out)


def closed_n(pos_y=K1.POS_Y):
    return 1.0 / (18.0 + 2.0 * pos_y)


def closed_pt_central(pos_x=K1.POS_X, pos_y=K1.POS_Y, grid=K1.GRID, h=1e-6):
    """dT/dxs by the central difference of ttgrid_ref.vert_T in the position"""
    import ttgrid_ref as G
    X, Y = K1.grid_xy(grid)
    return np.stack([(G.vert_T(xs + h, pos_y, X, Y) - G.vert_T(xs - h, pos_y, X, Y)) / (2 * h) for xs in pos_x])


# ------------------------------------------------------------------------------------------------ the acceptance case
ACC_HW = (0, 1, 2, 4, 8, 16)
ACC_COLS, ACC_REFLECTOR, ACC_ARTEFACT = slice(60, 141), slice(55, 66), slice(0, 45)


def acceptance_data():
    """-> (isrc, irec, data [48, NT], amid): the zero-offset section of the flat reflector m[60, :] = 1 over the 48 standard
    positions, each trace convolved with the 81-tap 60 Hz Ricker"""
    idx = np.arange(len(K1.POS_X), dtype=np.int32)
    m = np.zeros((K1.GRID[5], K1.GRID[2]))
    m[60, :] = 1.0
    d = (K1.matrix(K1.closed_T(), idx, idx, K1.NT, K1.DT) @ m.reshape(-1)).reshape(len(idx), K1.NT)
    wav = K1.ricker(np.arange(-40, 41) * K1.DT)
    d = np.stack([np.convolve(tr, wav, mode="same") for tr in d])
    return idx, idx.copy(), d, float(K1.POS_X[1] - K1.POS_X[0])


def acceptance_figures(img):
    """-> (reflector, artefact): the mean over columns 60 .. 140 of max|I| over rows 55 .. 65, and the rms of rows 0 .. 44"""
    img = np.asarray(img).reshape(K1.GRID[5], K1.GRID[2])
    reflector = float(np.mean(np.max(np.abs(img[ACC_REFLECTOR, ACC_COLS]), axis=0)))
    artefact = float(np.sqrt(np.mean(img[ACC_ARTEFACT, ACC_COLS] ** 2)))
    return reflector, artefact


# ------------------------------------------------------------------------------------------------ the small random case
SM_A = dict(asrc=0.02, arec=0.01, amid=0.015)


def small_case(karr, hw=HW8, pt_holes=False, lengths=SM_A, seed=0, **kw):
    """kirchhoff_multi_ref.small_case and, for it, -> (T, pt, aa, isrc, irec, kwargs): a quarter of the pt are exactly 0 (level 0
    needs a slope of exactly 0), the others spread the slope over 0.1 .. 160 samples per trace: every level of HW8 and beyond"""
    T, isrc, irec, k = KM.small_case(karr, seed=seed, **kw)
    rng = np.random.default_rng(1000 + seed)
    mag = KM.SM_DT / 0.01 * 10.0 ** rng.uniform(-1.0, 2.2, T.shape)
    pt = np.where(rng.random(T.shape) < 0.25, 0.0, rng.choice([-1.0, 1.0], T.shape) * mag)
    if pt_holes:
        pt = K1.with_holes(pt, rng)
        pt[rng.random(T.shape) < 0.01] = np.inf
    return T, pt, dict(hw=tuple(hw), **lengths), isrc, irec, k


def levels_hit(T, pt, aa, isrc, irec, nt, kw):
    """the set of levels the contributing pairs select, and whether a pair is steeper than the last level"""
    seen, beyond = set(), False
    Karr = T.shape[1]
    for k in range(len(isrc)):
        for ks in range(Karr):
            for kr in range(Karr):
                x = pair_terms(T, pt, aa, isrc[k], ks, irec[k], kr, None, nt, KM.SM_DT, amp=kw["amp"], theta=kw["theta"],
                               kmah=kw["kmah"], nbin=kw["nbin"], dopen=kw["dopen"])
                seen |= set(np.unique(x[6]).tolist())
                ps, pr = pt[isrc[k], ks].reshape(-1)[x[0]], pt[irec[k], kr].reshape(-1)[x[0]]
                sl = np.fmax(np.fmax(np.abs(ps) * aa["asrc"], np.abs(pr) * aa["arec"]), np.abs(ps + pr) * aa["amid"]) * (1.0 / KM.SM_DT)
                beyond = beyond or bool(np.any(sl > aa["hw"][-1]))
    return seen, beyond
