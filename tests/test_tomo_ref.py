"""CPU: the restatement of the compiled tomography matrix (tests/tomo_ref.py; include/rtmi.h) on the rows of a
golden trajectory: its segments, summed into a CSR matrix, are sensitivity_ref's A at the ends and at a line; its products are
the CSR's; the stacked operator with smoothing is its own adjoint; its solver agrees with scipy's lsqr on the same stacked
matrix.  rt_tomo.h, the storage layout, as a program of its own, plain and under -fsanitize=address,undefined.  The entries'
argument errors that need no device.  No GPU involved; tests/test_gpu_tomo.py compares the device with this restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT

import sensitivity_ref as S
import tomo_ref as TR

GOLD = os.path.join(ROOT, "tests", "golden")
LINE = (1.0, 0.0, 2.0)


@pytest.fixture(scope="module")
def rows():
    """every 64th row of the reference's vert_heterogeneous op6 fan as a record of its own, and the field's sample axes"""
    t = np.load(os.path.join(GOLD, "traj_vert_op6.npz"))
    f = np.load(os.path.join(GOLD, "field_vert_heterogeneous.npz"))
    s = t["strided"]
    last = np.minimum(t["d_ray"][2].astype(np.int64) // int(t["stride"]), s.shape[0] - 1)
    lim = f["limits"]
    qx, qy = int(f["qx"]), int(f["qy"])
    ax, ay = S.axes(np.linspace(lim[0], lim[1], qx), np.linspace(lim[2], lim[3], qy))
    return s, last, ax, ay, qx, qy


def test_segments_sum_to_the_sensitivity_matrix(rows):
    s, last, ax, ay, qx, qy = rows
    R = s.shape[2]
    M = S.matrices(s, last, ax, ay, line=LINE, kmax=2)
    nseg, rp, base, val = TR.segments(s, last, ax, ay)
    A = TR.to_csr(rp, base, val, qx, qy)
    big = abs(M["end"]).max()
    e_end = abs(A - M["end"]).max() / big
    assert np.array_equal(nseg, np.diff(rp)) and nseg.min() >= 1
    which = np.zeros(R, dtype=np.int64)
    nseg0, rp0, base0, val0 = TR.segments(s, last, ax, ay, which=which, line=LINE, kmax=2)
    A0 = TR.to_csr(rp0, base0, val0, qx, qy)
    e_line = abs(A0 - M["line"][:R]).max() / abs(M["line"][:R]).max()
    print(f"segments against sensitivity_ref: ends {e_end:.2e}, crossing 0 {e_line:.2e} of the largest entry; "
          f"{rp[-1]} and {rp0[-1]} segments, {int((M['count'] >= 1).sum())} rays cross")
    assert (M["count"] >= 1).sum() >= 8
    assert np.array_equal(nseg0 > 0, M["count"] >= 1)                        # no crossing: an empty row
    assert e_end <= 1e-13 and e_line <= 1e-13


def test_skipped_rays_have_no_row_and_a_missing_crossing_an_empty_one(rows):
    s, last, ax, ay, qx, qy = rows
    R = s.shape[2]
    which = np.full(R, -1)
    which[::3] = TR.SKIP
    which[1::3] = 5                                                          # no ray crosses the line six times
    nseg, rp, base, val = TR.segments(s, last, ax, ay, which=which, line=LINE, kmax=8)
    assert np.array_equal(nseg[::3], np.full(len(nseg[::3]), -1)) and not nseg[1::3].any() and nseg[2::3].min() >= 1
    assert len(rp) - 1 == int((which != TR.SKIP).sum()) and rp[-1] == len(base) == nseg[nseg > 0].sum()


def test_products_are_the_csr_matrix_products(rows):
    s, last, ax, ay, qx, qy = rows
    _, rp, base, val = TR.segments(s, last, ax, ay)
    A = TR.to_csr(rp, base, val, qx, qy)
    rng = np.random.default_rng(3)
    x = rng.standard_normal(qx * qy)
    w = rng.standard_normal(len(rp) - 1)
    y, yr = TR.apply(rp, base, val, qx, x), A @ x
    g, gr = TR.transpose(rp, base, val, qx, qy, w), A.T @ w
    e_y, e_g = np.max(np.abs(y - yr)) / np.max(np.abs(yr)), np.max(np.abs(g - gr)) / np.max(np.abs(gr))
    print(f"restated products against the CSR's: A x {e_y:.2e}, A^T w {e_g:.2e}")
    assert e_y <= 1e-13 and e_g <= 1e-13
    assert not TR.transpose(rp, base, val, qx, qy, np.zeros(len(rp) - 1)).any()


def stacked_matrix(A, qx, qy, lx, ly):
    n = qx * qy
    idx = np.arange(n).reshape(qy, qx)
    def diff(a, b, lam):
        m = a.size
        return sp.coo_matrix((np.r_[np.full(m, lam), np.full(m, -lam)], (np.r_[np.arange(m), np.arange(m)], np.r_[b.ravel(), a.ravel()])),
                             shape=(m, n)).tocsr()
    return sp.vstack([A, diff(idx[:, :-1], idx[:, 1:], lx), diff(idx[:-1, :], idx[1:, :], ly)]).tocsr()


def test_stacked_operator_is_its_own_adjoint(rows):
    s, last, ax, ay, qx, qy = rows
    _, rp, base, val = TR.segments(s, last, ax, ay)
    smooth = (0.5, 0.25)
    mv, rmv = TR.stacked(rp, base, val, qx, qy, smooth=smooth)
    rng = np.random.default_rng(5)
    x = rng.standard_normal(qx * qy)
    u = rng.standard_normal(len(rp) - 1 + qy * (qx - 1) + (qy - 1) * qx)
    Ax, Atu = mv(x), rmv(u)
    lhs, rhs = float(np.dot(Ax, u)), float(np.dot(x, Atu))
    scale = float(np.sum(np.abs(Ax * u)))
    print(f"stacked operator: <A x, u> - <x, A^T u> = {abs(lhs - rhs) / scale:.2e} relative")
    assert abs(lhs - rhs) <= 1e-12 * scale
    B = stacked_matrix(TR.to_csr(rp, base, val, qx, qy), qx, qy, *smooth)
    assert np.max(np.abs(Ax - B @ x)) <= 1e-13 * np.max(np.abs(Ax))
    assert np.max(np.abs(Atu - B.T @ u)) <= 1e-13 * np.max(np.abs(Atu))


@pytest.mark.parametrize("damp,smooth", [(0.0, None), (1e-3, (0.5, 0.25))])
def test_restated_solver_against_scipy(rows, damp, smooth):
    from scipy.sparse.linalg import lsqr
    s, last, ax, ay, qx, qy = rows
    _, rp, base, val = TR.segments(s, last, ax, ay)
    A = TR.to_csr(rp, base, val, qx, qy)
    rhs = np.random.default_rng(9).standard_normal(len(rp) - 1)
    out = TR.lsqr(rp, base, val, qx, qy, rhs, 8, damp=damp, smooth=smooth)
    B = A if smooth is None else stacked_matrix(A, qx, qy, *smooth)
    b = np.r_[rhs, np.zeros(B.shape[0] - len(rhs))]
    ref = lsqr(B, b, damp=damp, atol=0.0, btol=0.0, conlim=0.0, iter_lim=8)
    e1, e2 = abs(out["r1norm"] - ref[3]) / ref[3], abs(out["r2norm"] - ref[4]) / ref[4]
    print(f"damp {damp}, smooth {smooth}: itn {out['itn']} / {ref[2]}, r1norm {e1:.2e}, r2norm {e2:.2e} relative to scipy")
    assert out["itn"] == ref[2] == 8 and out["istop"] == ref[1] == 7
    assert e1 <= 1e-6 and e2 <= 1e-6
    assert np.max(np.abs(out["x"].ravel() - ref[0])) <= 1e-6 * np.max(np.abs(ref[0]))


# ---------------------------------------------------------------- rt_tomo.h as a program
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("tomo_layout")
    src = os.path.join(ROOT, "tests", "native", "tomo_layout.cpp")
    out = {}
    for name, flags in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + flags + ["-o", exe, src])
        out[name] = exe
    return out


def lengths(rows, seed):
    """rows of 0, 1 and a few hundred segments side by side"""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 6, rows)
    n[rng.random(rows) < 0.1] = 0
    n[rng.random(rows) < 0.05] = 300
    return n


BLOCKS = [[0], [1], [63], [64], [65], [129], [65, 0, 1, 129, 64]]


@pytest.mark.parametrize("build", ["plain", "san"])
@pytest.mark.parametrize("blocks", BLOCKS, ids=lambda b: "+".join(map(str, b)))
def test_layout_program(programs, build, blocks):
    lens = [lengths(r, 10 * i + r) for i, r in enumerate(blocks)]
    text = f"{len(blocks)}\n" + "".join(f"{len(n)} " + " ".join(map(str, n)) + "\n" for n in lens)
    r = subprocess.run([programs[build]], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1].split() == ["rows", str(sum(blocks))]
    at, first = 0, 0
    for n in lens:
        head = lines[at].split()
        ns = (len(n) + 63) // 64
        widths = [int(n[64 * s_:64 * s_ + 64].max()) for s_ in range(ns)]
        off = np.r_[0, np.cumsum([64 * w for w in widths])].astype(np.int64)
        assert head[:5] == ["block", str(first), str(len(n)), str(int(n.sum())), str(int(off[-1]))] and head[5] == "off"
        assert [int(v) for v in head[6:]] == off.tolist()
        for r_ in range(len(n)):
            _, g, slot, value = lines[at + 1 + r_].split()
            o = off[r_ // 64]
            want = (o + r_ % 64, 4 * o + 64 * 3 + r_ % 64) if n[r_] else (-1, -1)
            assert (int(g), int(slot), int(value)) == (first + r_,) + want
        at += 1 + len(n)
        first += len(n)


# ---------------------------------------------------------------- argument errors that need no device
def test_argument_errors_need_no_device():
    from raytracing_amd import _lib
    L = _lib.lib()
    st, ls, lp = _lib.TomoStats(), _lib.LsqrStats(), _lib.LsqrParams()
    lp.iter_lim = 1
    h = C.c_void_p()
    first = C.c_int64()
    x = np.zeros(4)
    calls = {
        "rtmi_tomo_create: null field": lambda: L.rtmi_tomo_create(None, C.byref(h)),
        "rtmi_tomo_append: null handle": lambda: L.rtmi_tomo_append(None, None, None, 0, None, None, C.byref(first)),
        "rtmi_tomo_read: null handle": lambda: L.rtmi_tomo_read(None, None, None, None),
        "rtmi_tomo_info: null handle": lambda: L.rtmi_tomo_info(None, C.byref(st)),
        "rtmi_tomo_apply: null handle": lambda: L.rtmi_tomo_apply(None, _lib.dptr(x), _lib.dptr(x), None),
        "rtmi_tomo_apply_dev: null handle": lambda: L.rtmi_tomo_apply_dev(None, None, None, None),
        "rtmi_tomo_transpose: null handle": lambda: L.rtmi_tomo_transpose(None, _lib.dptr(x), _lib.dptr(x), None),
        "rtmi_tomo_transpose_dev: null handle": lambda: L.rtmi_tomo_transpose_dev(None, None, None, None),
        "rtmi_tomo_lsqr: null handle": lambda: L.rtmi_tomo_lsqr(None, C.byref(lp), None, _lib.dptr(x), _lib.dptr(x), None, C.byref(ls)),
    }
    for msg, call in calls.items():
        assert call() == -1, msg                                             # RTMI_ERR_ARG
        assert L.rtmi_last_error().decode() == msg
    L.rtmi_tomo_destroy(None)                                                # a no-op, as free(NULL)
