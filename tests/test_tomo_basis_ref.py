"""CPU: the restatement of the tomography model basis (tests/tomo_basis_ref.py; include/rtmi.h).
rtmi_bspline_axis against the restatement bit for bit and against the exact rational weights; the restated operator pair against
a dense matrix built from the weights, and their adjointness; the stacked operator with both regularisers against its own
adjoint; the restated solver against scipy's lsqr on the dense A P stacked with the regulariser; rt_tomo_basis.h as a program
of its own, plain and under -fsanitize=address,undefined; the new entries' argument errors that need no device; the size of
rtmi_tomo_reg.  No GPU involved; tests/test_gpu_tomo_basis.py compares the device with this restatement."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT

import sensitivity_ref as S
import tomo_basis_ref as BR
import tomo_ref as TR

GOLD = os.path.join(ROOT, "tests", "golden")
SHAPES = [(2, None), (5, None), (37, 7), (64, 9), (65, 33), (9, "9+d")]          # None: m = degree + 1


def shape(q, m, d):
    return q, (d + 1 if m is None else 9 + d if m == "9+d" else m)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def exact_weights(q, m, d):
    """the B-spline weights as exact rationals"""
    n = m if d == 0 else m - d
    out = []
    for j in range(q):
        e = min(j * n // (q - 1), n - 1)
        t = Fraction(j * n - e * (q - 1), q - 1)
        u = 1 - t
        out.append([Fraction(1)] if d == 0 else [u, t] if d == 1 else
                   [u ** 3 / 6, ((3 * t - 6) * t * t + 4) / 6, (((-3 * t + 3) * t + 3) * t + 1) / 6, t ** 3 / 6])
    return out


def ulps(have, want):
    """|have - want| in units of the spacing of fp64 at want (a Fraction)"""
    if want == 0:
        return 0.0 if have == 0.0 else np.inf
    return float(abs(Fraction(have) - want) / Fraction(float(np.spacing(abs(float(want))))))


# ---------------------------------------------------------------- rtmi_bspline_axis
@pytest.mark.parametrize("d", [0, 1, 3])
@pytest.mark.parametrize("qm", SHAPES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_bspline_axis_equals_the_restatement_and_the_exact_weights(d, qm):
    from raytracing_amd import rt_bench as rb
    q, m = shape(*qm, d)
    first, wgt = rb.bspline_axis(q, m, d)
    rf, rw = BR.bspline_axis(q, m, d)
    assert first.dtype == np.int32 and wgt.shape == (q, d + 1)
    assert np.array_equal(first, rf) and bits(wgt) == bits(rw)
    assert (np.diff(first) >= 0).all() and first.min() >= 0 and first.max() <= m - (d + 1)
    exact = exact_weights(q, m, d)
    worst = max(ulps(float(wgt[j, b]), exact[j][b]) for j in range(q) for b in range(d + 1))
    unit = float(np.max(np.abs(wgt.sum(axis=1) - 1.0)))
    print(f"degree {d}, q {q}, m {m}: {worst:.2f} ulp from the exact weights, |sum - 1| {unit:.2e}")
    assert worst <= 1.0
    assert unit <= 4.5e-16
    if d == 0 and m == q:
        assert np.array_equal(first, np.arange(q))


def test_degree_0_with_m_equal_to_q_is_the_identity():
    from raytracing_amd import rt_bench as rb
    first, wgt = rb.bspline_axis(9, 9, 0)
    assert np.array_equal(first, np.arange(9)) and np.array_equal(wgt, np.ones((9, 1)))


# ---------------------------------------------------------------- the restated operator
def small_basis():
    """cubic x linear on 23 x 37 onto 6 x 7: qx 37, qy 23, mx 7, my 6"""
    return BR.Basis.bspline(37, 23, 7, 6, degree=(3, 1))


def caller_axis():
    """a caller-made axis with B = 2 on q = 12, m = 9: repeated first, a jump of B, zero weights, and coefficient 5 unreached"""
    first = np.array([0, 0, 0, 1, 1, 3, 3, 3, 6, 6, 7, 7], dtype=np.int32)
    rng = np.random.default_rng(77)
    wgt = rng.standard_normal((12, 2))
    wgt[2] = 0.0
    wgt[6, 1] = 0.0
    return first, wgt, 9


def test_restated_operator_against_a_dense_matrix():
    rng = np.random.default_rng(1)
    fx, wx, mx = caller_axis()
    for B in (small_basis(), BR.Basis(fx, wx, *BR.bspline_axis(23, 6, 1), mx, 6)):
        P = B.dense()
        c = rng.standard_normal((B.my, B.mx))
        x = rng.standard_normal((B.qy, B.qx))
        e_p = np.abs(B.prolong(c).ravel() - P @ c.ravel()) / (np.abs(P) @ np.abs(c.ravel()) + 1e-300)
        e_r = np.abs(B.restrict(x).ravel() - P.T @ x.ravel()) / (np.abs(P.T) @ np.abs(x.ravel()) + 1e-300)
        print(f"restated P and P^T against the dense matrix: {e_p.max():.2e}, {e_r.max():.2e} of sum |terms|")
        assert e_p.max() <= 1e-15 and e_r.max() <= 1e-15
    assert not B.restrict(x)[:, 5].any() and not np.signbit(B.restrict(x)[:, 5]).any()      # the unreached coefficient


def test_restated_pair_is_adjoint_and_reproduces_constants():
    rng = np.random.default_rng(2)
    B = small_basis()
    c = rng.standard_normal((B.my, B.mx))
    x = rng.standard_normal((B.qy, B.qx))
    Pc, Ptx = B.prolong(c), B.restrict(x)
    lhs, rhs = float(np.sum(Pc * x)), float(np.sum(c * Ptx))
    scale = float(np.abs(x.ravel()) @ np.abs(B.dense()) @ np.abs(c.ravel()))
    one = float(np.max(np.abs(B.prolong(np.ones((B.my, B.mx))) - 1.0)))
    print(f"<P c, x> - <c, P^T x> = {abs(lhs - rhs) / scale:.2e} of sum |terms|; |P 1 - 1| {one:.2e}")
    assert abs(lhs - rhs) <= 1e-15 * scale
    assert one <= 4.5e-16


def test_ranges_are_the_definition():
    fx, wx, mx = caller_axis()
    lo, hi = BR.ranges(fx, mx, 2)
    for l in range(mx):
        reach = [j for j in range(len(fx)) if 0 <= l - fx[j] < 2]
        assert reach == list(range(lo[l], hi[l])), l
    assert lo[5] == hi[5]


# ---------------------------------------------------------------- the stacked operator and the solver, on a golden trajectory
@pytest.fixture(scope="module")
def rows():
    """tests/test_tomo_ref.py's: every 64th row of the reference's vert_heterogeneous op6 fan as a record of its own"""
    t = np.load(os.path.join(GOLD, "traj_vert_op6.npz"))
    f = np.load(os.path.join(GOLD, "field_vert_heterogeneous.npz"))
    s = t["strided"]
    last = np.minimum(t["d_ray"][2].astype(np.int64) // int(t["stride"]), s.shape[0] - 1)
    lim = f["limits"]
    qx, qy = int(f["qx"]), int(f["qy"])
    ax, ay = S.axes(np.linspace(lim[0], lim[1], qx), np.linspace(lim[2], lim[3], qy))
    _, rp, base, val = TR.segments(s, last, ax, ay)
    return rp, base, val, qx, qy


def reg_matrix(gx, gy, d1, d2):
    n = gx * gy
    idx = np.arange(n).reshape(gy, gx)

    def rowsof(terms, m):
        r = np.concatenate([np.arange(m)] * len(terms))
        return sp.coo_matrix((np.concatenate([np.full(m, v) for _, v in terms]), (r, np.concatenate([c.ravel() for c, _ in terms]))),
                             shape=(m, n)).tocsr()
    parts = []
    if d1 is not None:
        parts += [rowsof([(idx[:, 1:], d1[0]), (idx[:, :-1], -d1[0])], gy * (gx - 1)),
                  rowsof([(idx[1:, :], d1[1]), (idx[:-1, :], -d1[1])], (gy - 1) * gx)]
    if d2 is not None:
        parts += [rowsof([(idx[:, :-2], d2[0]), (idx[:, 2:], d2[0]), (idx[:, 1:-1], -2 * d2[0])], gy * (gx - 2)),
                  rowsof([(idx[:-2, :], d2[1]), (idx[2:, :], d2[1]), (idx[1:-1, :], -2 * d2[1])], (gy - 2) * gx)]
    return sp.vstack(parts).tocsr()


@pytest.mark.parametrize("with_basis", [True, False])
def test_stacked_operator_with_both_regularisers_is_its_own_adjoint(rows, with_basis):
    rp, base, val, qx, qy = rows
    B = BR.Basis.bspline(qx, qy, 9, 7) if with_basis else None
    gx, gy = (9, 7) if with_basis else (qx, qy)
    d1, d2 = (0.5, 0.25), (0.3, 0.2)
    mv, rmv, nr = BR.stacked(rp, base, val, qx, qy, basis=B, d1=d1, d2=d2)
    assert nr == gy * (gx - 1) + (gy - 1) * gx + gy * (gx - 2) + (gy - 2) * gx
    rng = np.random.default_rng(5)
    s = rng.standard_normal(gx * gy)
    u = rng.standard_normal(len(rp) - 1 + nr)
    As, Atu = mv(s), rmv(u)
    lhs, rhs = float(np.dot(As, u)), float(np.dot(s, Atu))
    scale = float(np.sum(np.abs(As * u)))
    print(f"stacked operator, basis {with_basis}: <A s, u> - <s, A^T u> = {abs(lhs - rhs) / scale:.2e} relative")
    assert abs(lhs - rhs) <= 1e-12 * scale
    R = reg_matrix(gx, gy, d1, d2)
    rows_ = len(rp) - 1
    assert np.max(np.abs(As[rows_:] - R @ s)) <= 1e-13 * np.max(np.abs(As[rows_:]))
    g0 = rmv(np.r_[u[:rows_], np.zeros(nr)])
    assert np.max(np.abs((Atu - g0) - R.T @ u[rows_:])) <= 1e-13 * np.max(np.abs(Atu))


@pytest.mark.parametrize("iters,damp,d1,d2", [(30, 1e-3, (0.5, 0.25), (0.3, 0.2)), (30, 0.0, (0.5, 0.25), (0.3, 0.2)),
                                              (8, 0.0, None, None), (8, 0.0, None, (0.3, 0.2)), (8, 1e-3, (0.5, 0.25), None)])
def test_restated_basis_solver_against_scipy(rows, iters, damp, d1, d2):
    """30 iterations with the regulariser stacked, d1 and d2 together; 8 iterations, the count of
    test_tomo_ref.py::test_restated_solver_against_scipy, for the other combinations.  The golden fan has 31 rays, so A P is 31 x 63
    with singular values from 5.8 to 4.7e-5.  LSQR does not re-orthogonalise: two runs that differ only in how sums are rounded
    drift apart as the iteration goes on.  scipy against itself on a matrix perturbed by one ulp per entry, 30 iterations, differs by
    6e-8 (d1 and d2, damp 1e-3), 5e-8 (d1 and d2, damp 0), 1e-4 (d1 or d2 alone) and 1e-3 (no regulariser: 30 iterations exhaust
    the 31 rows) of the largest value: only with both regularisers is the reference itself defined to 1e-6 at 30 iterations.
    At 8 iterations the restatement and scipy agree to 1e-10 in every combination."""
    from scipy.sparse.linalg import lsqr
    rp, base, val, qx, qy = rows
    B = BR.Basis.bspline(qx, qy, 9, 7)
    A = TR.to_csr(rp, base, val, qx, qy)
    P = sp.kron(sp.csr_matrix(B.axis_matrix("y")), sp.csr_matrix(B.axis_matrix("x"))).tocsr()
    AP = (A @ P).toarray()
    rhs = np.random.default_rng(9).standard_normal(len(rp) - 1)
    out = BR.lsqr(rp, base, val, qx, qy, rhs, iters, basis=B, d1=d1, d2=d2, damp=damp)
    M = AP if d1 is None and d2 is None else np.vstack([AP, reg_matrix(9, 7, d1, d2).toarray()])
    b = np.r_[rhs, np.zeros(M.shape[0] - len(rhs))]
    ref = lsqr(M, b, damp=damp, atol=0.0, btol=0.0, conlim=0.0, iter_lim=iters)
    e = float(np.max(np.abs(out["c"].ravel() - ref[0])) / np.max(np.abs(ref[0])))
    ex = float(np.max(np.abs(out["x"].ravel() - P @ ref[0])) / np.max(np.abs(P @ ref[0])))
    print(f"{iters} iterations, damp {damp}, d1 {d1}, d2 {d2}: itn {out['itn']} / {ref[2]}, c {e:.2e}, x {ex:.2e} of the largest value against scipy")
    assert out["itn"] == ref[2] == iters and out["istop"] == ref[1] == 7
    assert e <= 1e-6 and ex <= 1e-6


# ---------------------------------------------------------------- rt_tomo_basis.h as a program
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("tomo_basis_check")
    src = os.path.join(ROOT, "tests", "native", "tomo_basis_check.cpp")
    out = {}
    for name, flags in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + flags + ["-o", exe, src])
        out[name] = exe
    return out


def axis_text(which, first, wgt, m):
    wgt = np.asarray(wgt, dtype=np.float64).reshape(len(first), -1)
    return f"axis {which} {len(first)} {m} {wgt.shape[1]}\n" + "".join(
        f"{int(f)} " + " ".join(float(v).hex() for v in w) + "\n" for f, w in zip(first, wgt))


def run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    return r.stdout.splitlines()


def hexes(line, name):
    tok = line.split()
    assert tok[0] == name
    return np.array([float.fromhex(v) for v in tok[1:]])


@pytest.mark.parametrize("build", ["plain", "san"])
def test_header_program_axes_ranges_and_pair(programs, build):
    fx, wx, mx = caller_axis()                                               # repeats, a jump of B, an unreached coefficient
    fy = np.array([0, 0, 0, 0], dtype=np.int32)                              # m = B: every sample on the same B coefficients
    wy = np.random.default_rng(3).standard_normal((4, 3))
    B = BR.Basis(fx, wx, fy, wy, mx, 3)
    rng = np.random.default_rng(4)
    c, x = rng.standard_normal((B.my, B.mx)), rng.standard_normal((B.qy, B.qx))
    text = axis_text("x", fx, wx, mx) + axis_text("y", fy, wy, 3) + "pair\n" + " ".join(float(v).hex() for v in np.r_[c.ravel(), x.ravel()]) + "\n"
    out = run(programs[build], text)
    assert out[0] == "axis ok" and out[3] == "axis ok"
    assert [int(v) for v in out[1].split()[1:]] == B.lox.tolist() and [int(v) for v in out[2].split()[1:]] == B.hix.tolist()
    assert [int(v) for v in out[4].split()[1:]] == B.loy.tolist() == [0, 0, 0] and [int(v) for v in out[5].split()[1:]] == B.hiy.tolist() == [4, 4, 4]
    assert bits(hexes(out[6], "prolong")) == bits(B.prolong(c)) and bits(hexes(out[7], "restrict")) == bits(B.restrict(x))


@pytest.mark.parametrize("build", ["plain", "san"])
def test_header_program_refuses_bad_axes(programs, build):
    ok_w = np.ones((4, 2))
    nan_w = ok_w.copy(); nan_w[2, 1] = np.nan
    cases = [((np.array([0, 1, 0, 1]), ok_w, 3), "axis bad 2 first decreases"),
             ((np.array([0, 1, 1, 2]), ok_w, 3), "axis bad 3 first is outside 0 .. m - B"),
             ((np.array([-1, 0, 0, 1]), ok_w, 3), "axis bad 0 first is outside 0 .. m - B"),
             ((np.array([0, 0, 1, 1]), nan_w, 3), "axis bad 2 a weight is not finite"),
             ((np.array([0, 0, 0, 0]), ok_w, 1), "axis bad -1 fewer coefficients than the bandwidth"),
             ((np.array([0, 0, 0, 0]), np.ones((4, 5)), 9), "axis bad -1 the bandwidth must be in 1 .. 4")]
    text = "".join(axis_text("x", *a) for a, _ in cases)
    assert run(programs[build], text) == [msg for _, msg in cases]


@pytest.mark.parametrize("build", ["plain", "san"])
def test_header_program_bspline_weights(programs, build):
    cases = [(d,) + shape(*qm, d) for d in (0, 1, 3) for qm in SHAPES]
    text = "".join(f"bspline {q} {m} {d}\n" for d, q, m in cases) + "bspline 1 4 3\nbspline 9 3 3\nbspline 9 9 2\n"
    out = run(programs[build], text)
    at = 0
    for d, q, m in cases:
        assert out[at] == "bspline ok"
        first, wgt = BR.bspline_axis(q, m, d)
        for j in range(q):
            tok = out[at + 1 + j].split()
            assert int(tok[0]) == first[j] and bits([float.fromhex(v) for v in tok[1:]]) == bits(wgt[j]), (d, q, m, j)
        at += 1 + q
    assert out[at:] == ["bspline refused"] * 3


# ---------------------------------------------------------------- argument errors that need no device, and the ABI
def test_argument_errors_need_no_device():
    from raytracing_amd import _lib
    L = _lib.lib()
    ls, lp = _lib.LsqrStats(), _lib.LsqrParams()
    lp.iter_lim = 1
    h = C.c_void_p()
    x = np.zeros(4)
    f = np.zeros(4, dtype=np.int32)
    ip = f.ctypes.data_as(_lib._ip)
    fake = C.c_void_p(8)                                                     # never dereferenced: a null argument comes first
    calls = {
        "rtmi_bspline_axis: null first": lambda: L.rtmi_bspline_axis(4, 4, 3, None, _lib.dptr(x)),
        "rtmi_bspline_axis: null wgt": lambda: L.rtmi_bspline_axis(4, 4, 3, ip, None),
        "rtmi_bspline_axis: degree must be 0, 1 or 3": lambda: L.rtmi_bspline_axis(4, 4, 2, ip, _lib.dptr(x)),
        "rtmi_bspline_axis: q must be >= 2": lambda: L.rtmi_bspline_axis(1, 4, 3, ip, _lib.dptr(x)),
        "rtmi_bspline_axis: m must be >= degree + 1": lambda: L.rtmi_bspline_axis(4, 3, 3, ip, _lib.dptr(x)),
        "rtmi_tomo_basis_create: null handle": lambda: L.rtmi_tomo_basis_create(None, 1, 1, ip, _lib.dptr(x), 1, 1, ip, _lib.dptr(x), C.byref(h)),
        "rtmi_tomo_basis_create: null first_x": lambda: L.rtmi_tomo_basis_create(fake, 1, 1, None, _lib.dptr(x), 1, 1, ip, _lib.dptr(x), C.byref(h)),
        "rtmi_tomo_basis_create: null wgt_x": lambda: L.rtmi_tomo_basis_create(fake, 1, 1, ip, None, 1, 1, ip, _lib.dptr(x), C.byref(h)),
        "rtmi_tomo_basis_create: null first_y": lambda: L.rtmi_tomo_basis_create(fake, 1, 1, ip, _lib.dptr(x), 1, 1, None, _lib.dptr(x), C.byref(h)),
        "rtmi_tomo_basis_create: null wgt_y": lambda: L.rtmi_tomo_basis_create(fake, 1, 1, ip, _lib.dptr(x), 1, 1, ip, None, C.byref(h)),
        "rtmi_tomo_basis_create: null out": lambda: L.rtmi_tomo_basis_create(fake, 1, 1, ip, _lib.dptr(x), 1, 1, ip, _lib.dptr(x), None),
        "rtmi_tomo_basis_prolong: null handle": lambda: L.rtmi_tomo_basis_prolong(None, _lib.dptr(x), _lib.dptr(x)),
        "rtmi_tomo_basis_prolong: null c": lambda: L.rtmi_tomo_basis_prolong(fake, None, _lib.dptr(x)),
        "rtmi_tomo_basis_prolong: null x": lambda: L.rtmi_tomo_basis_prolong(fake, _lib.dptr(x), None),
        "rtmi_tomo_basis_restrict: null handle": lambda: L.rtmi_tomo_basis_restrict(None, _lib.dptr(x), _lib.dptr(x)),
        "rtmi_tomo_basis_restrict: null x": lambda: L.rtmi_tomo_basis_restrict(fake, None, _lib.dptr(x)),
        "rtmi_tomo_basis_restrict: null g": lambda: L.rtmi_tomo_basis_restrict(fake, _lib.dptr(x), None),
        "rtmi_tomo_basis_prolong_dev: null handle": lambda: L.rtmi_tomo_basis_prolong_dev(None, None, None),
        "rtmi_tomo_basis_prolong_dev: null d_c": lambda: L.rtmi_tomo_basis_prolong_dev(fake, None, fake),
        "rtmi_tomo_basis_prolong_dev: null d_x": lambda: L.rtmi_tomo_basis_prolong_dev(fake, fake, None),
        "rtmi_tomo_basis_restrict_dev: null handle": lambda: L.rtmi_tomo_basis_restrict_dev(None, None, None),
        "rtmi_tomo_basis_restrict_dev: null d_x": lambda: L.rtmi_tomo_basis_restrict_dev(fake, None, fake),
        "rtmi_tomo_basis_restrict_dev: null d_g": lambda: L.rtmi_tomo_basis_restrict_dev(fake, fake, None),
        "rtmi_tomo_lsqr_basis: null handle": lambda: L.rtmi_tomo_lsqr_basis(None, None, C.byref(lp), None, None, _lib.dptr(x), None, _lib.dptr(x),
                                                                           None, C.byref(ls)),
    }
    for msg, call in calls.items():
        assert call() == -1, msg                                             # RTMI_ERR_ARG
        assert L.rtmi_last_error().decode() == msg
    L.rtmi_tomo_basis_destroy(None)                                          # a no-op, as free(NULL)


def test_abi_version_and_struct_size(tmp_path):
    from raytracing_amd import _lib
    assert _lib.lib().rtmi_abi_version() == _lib.ABI_VERSION == 7
    src = tmp_path / "sz.c"
    src.write_text('#include "rtmi.h"\n#include <stdio.h>\nint main(void){printf("%zu\\n", sizeof(rtmi_tomo_reg)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert int(subprocess.check_output([str(exe)]).decode()) == C.sizeof(_lib.TomoReg) == 64
