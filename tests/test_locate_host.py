"""CPU: event location by grid search (rtmi_locator_*, rtmi_locate, rtmi_locate_dev).  The entries and the
cap are declared, exported and bound with the header's signatures, the structs have gcc's sizes and the ABI version stays 7; the
refusals that need no device come before any device work and name the argument; rt_locate.h as a program of its own
(tests/native/locate_refine.cpp, plain and under the sanitizers) agrees with tests/locate_ref.py bit for bit on the refinement --
accepted, saddle, det = 0, a step over one cell, one NaN -- and on a node's two passes; the restatement finds the truth on
closed-form tables.  What needs a handle is in tests/test_gpu_locate.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import locate_ref
from conftest import ROOT
from raytracing_amd import _lib, rt_bench

_dp = C.POINTER(C.c_double)
NAMES = ("rtmi_locator_create", "rtmi_locator_destroy", "rtmi_locate", "rtmi_locate_dev")


def _prototype(name, ret="int"):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtmi.h")).read(), flags=re.S)
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entries():
    assert _prototype("rtmi_locator_create") == ["const rtmi_locator_params *lp", "const double *T", "rtmi_locator **out"]
    assert _prototype("rtmi_locator_destroy", "void") == ["rtmi_locator *loc"]
    assert _prototype("rtmi_locate") == ["rtmi_locator *loc", "int64_t E", "const double *t", "const double *w", "const int32_t *need",
                                         "rtmi_locate_result *res", "double *maps", "rtmi_locate_stats *st"]
    assert _prototype("rtmi_locate_dev") == ["rtmi_locator *loc", "int64_t E", "const double *d_t", "const double *d_w",
                                             "const int32_t *d_need", "rtmi_locate_result *res", "double *d_maps", "rtmi_locate_stats *st"]
    src = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert re.search(r"#define\s+RTMI_LOCATE_MAX_TABLES\s+512\b", src) and _lib.LOCATE_MAX_TABLES == 512
    assert re.search(r"#define\s+RTMI_ABI_VERSION\s+7\b", src)


def test_ctypes_signatures_and_exports():
    res, st = C.POINTER(_lib.LocateResult), C.POINTER(_lib.LocateStats)
    assert _lib.SYMBOLS["rtmi_locator_create"] == (C.c_int, [C.POINTER(_lib.LocatorParams), _dp, C.POINTER(C.c_void_p)])
    assert _lib.SYMBOLS["rtmi_locator_destroy"] == (None, [C.c_void_p])
    assert _lib.SYMBOLS["rtmi_locate"] == (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp, _lib._ip, res, _dp, st])
    assert _lib.SYMBOLS["rtmi_locate_dev"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, res, C.c_void_p, st])
    _lib.lib()                                                                # first: it maps the HIP runtime the library shares with torch
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name)
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    assert _lib.lib().rtmi_abi_version() == 7 and _lib.ABI_VERSION == 7
    for name in ("from_table", "locate", "locate_device", "close"):
        assert callable(getattr(rt_bench.Locator, name))


def test_struct_sizes_match_gccs(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include "rtmi.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(rtmi_locator_params), sizeof(rtmi_locate_result), sizeof(rtmi_locate_stats), '
                   'offsetof(rtmi_locate_result, win_obj), offsetof(rtmi_locate_result, cov), offsetof(rtmi_locate_result, refined)); '
                   'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    R = _lib.LocateResult
    assert sizes == [C.sizeof(_lib.LocatorParams), C.sizeof(R), C.sizeof(_lib.LocateStats), R.win_obj.offset, R.cov.offset, R.refined.offset]


# ---------------------------------------------------------------- refusals without a device
FAKE = C.c_void_p(8)              # never dereferenced: the checks below come before the handle is read
BUF = (C.c_double * 8)()


def _refused(rc, who, *words):
    msg = _lib.lib().rtmi_last_error()
    assert rc == -1, msg
    assert msg.startswith(who.encode() + b": "), msg
    for w in words:
        assert w.encode() in msg, msg


def _params(nx=4, ny=2, P=1, gdx=1.0, gdy=1.0, gx0=0.0, gy0=0.0):
    lp = _lib.LocatorParams()
    lp.nx, lp.ny, lp.P, lp.gx0, lp.gdx, lp.gy0, lp.gdy = nx, ny, P, gx0, gdx, gy0, gdy
    return lp


def test_create_refusals_that_need_no_device():
    L = _lib.lib()
    who = "rtmi_locator_create"
    h = C.c_void_p(1)

    def call(lp, T=BUF, out=h):
        return L.rtmi_locator_create(None if lp is None else C.byref(lp), T, None if out is None else C.byref(out))

    _refused(call(_params(), out=None), who, "null out")
    _refused(call(None), who, "null lp")
    assert h.value is None                                   # a refused create leaves no handle
    _refused(call(_params(), T=None), who, "null T")
    for kw in (dict(nx=0), dict(ny=0), dict(nx=-3)):
        _refused(call(_params(**kw)), who, "nx and ny must be >= 1")
    for P in (0, -1):
        _refused(call(_params(P=P)), who, "P must be >= 1")
    for P in (513, 1 << 20):
        _refused(call(_params(P=P)), who, "P is over RTMI_LOCATE_MAX_TABLES")
    _refused(call(_params(nx=1 << 16, ny=(1 << 15) + 1)), who, "2^31")
    for kw in (dict(gdx=0.0), dict(gdy=-1.0), dict(gdx=float("nan")), dict(gdy=float("inf"))):
        _refused(call(_params(**kw)), who, "gdx and gdy must be finite and > 0")
    for kw in (dict(gx0=float("nan")), dict(gy0=float("inf"))):
        _refused(call(_params(**kw)), who, "gx0 and gy0 must be finite")


@pytest.mark.parametrize("name", ["rtmi_locate", "rtmi_locate_dev"])
def test_locate_refusals_that_need_no_device(name):
    fn = getattr(_lib.lib(), name)
    res = (_lib.LocateResult * 2)()
    p = C.c_void_p(64) if name.endswith("_dev") else BUF
    _refused(fn(None, 1, p, None, None, res, None, None), name, "null handle")
    _refused(fn(FAKE, 1, None, None, None, res, None, None), name, "null t")
    _refused(fn(FAKE, 1, p, None, None, None, None, None), name, "null res")
    for E in (0, -5):
        _refused(fn(FAKE, E, p, None, None, res, None, None), name, "E must be >= 1")


def test_python_checks_shapes_first():
    class Shape(rt_bench.Locator):
        def __init__(self):
            self.P, self.ny, self.nx, self.grid, self._h = 3, 4, 5, (0.0, 1.0, 5, 0.0, 1.0, 4), None

    S = Shape()
    with pytest.raises(ValueError, match=r"picks must be \[E, 3\]"):
        S.locate(np.zeros((2, 4)))
    with pytest.raises(ValueError, match="weights must have the shape of picks"):
        S.locate(np.zeros((2, 3)), weights=np.ones((2, 2)))
    with pytest.raises(RuntimeError, match="closed"):
        S.locate(np.zeros((2, 3)))
    with pytest.raises(ValueError, match=r"T must be \[P, ny, nx\]"):
        rt_bench.Locator(np.zeros((4, 5)), S.grid)
    with pytest.raises(ValueError, match="of the grid"):
        rt_bench.Locator(np.zeros((3, 5, 4)), S.grid)


# ---------------------------------------------------------------- rt_locate.h as a program
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("locate_refine")
    src = os.path.join(ROOT, "tests", "native", "locate_refine.cpp")
    out = {}
    for name, flags in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall"] + flags + ["-o", exe, src])
        out[name] = exe
    return out


def hx(v):
    return float(v).hex()


def unhx(s):
    return float("nan") if "nan" in s else float.fromhex(s)


GRID = (-2.0, 0.1, 37, -2.3, 0.25, 29)


def bowl(a, b, c, x0, y0, base=0.5):
    """f = base + a (x - x0)^2 + 2 b (x - x0)(y - y0) + c (y - y0)^2 on the window's nodes"""
    j, i = np.meshgrid((-1.0, 0.0, 1.0), (-1.0, 0.0, 1.0), indexing="ij")
    return base + a * (i - x0) ** 2 + 2 * b * (i - x0) * (j - y0) + c * (j - y0) ** 2


def windows():
    rng = np.random.default_rng(11)
    tau = lambda: 0.3 + 0.01 * rng.standard_normal((3, 3))                      # noqa: E731
    W = {"accepted": bowl(1.0, 0.2, 0.7, 0.31, -0.22), "accepted_noisy": bowl(1.3, -0.4, 0.9, -0.4, 0.45) + 1e-3 * rng.standard_normal((3, 3)),
         "saddle": bowl(1.0, 0.0, -0.8, 0.1, 0.1), "maximum": bowl(-1.0, 0.0, -1.0, 0.0, 0.0),
         "det_zero": bowl(1.0, 1.0, 1.0, 0.2, 0.1), "flat": np.full((3, 3), 0.25),
         "step_over_a_cell_x": bowl(1.0, 0.0, 1.0, 1.7, 0.0), "step_over_a_cell_y": bowl(1.0, 0.0, 1.0, 0.0, -1.2),
         "step_of_one_cell": bowl(1.0, 0.0, 1.0, 1.0, -1.0)}
    nan = W["accepted"].copy()
    nan[2, 0] = np.nan
    inf = W["accepted"].copy()
    inf[0, 1] = np.inf
    W["one_nan"], W["one_inf"] = nan, inf
    return [(k, f, tau()) for k, f in W.items()]


@pytest.mark.parametrize("which", ["plain", "san"])
def test_refinement_program_agrees_with_the_restatement_bit_for_bit(programs, which):
    cases = windows()
    text = ""
    for k, (_, f, tau) in enumerate(cases):
        text += "refine " + " ".join(hx(v) for v in f.ravel()) + " " + " ".join(hx(v) for v in tau.ravel())
        text += f" {hx(1e5 + k)} {hx(7.0 + k)} {3 + k} {20 - k} " + " ".join(hx(GRID[q]) for q in (0, 1, 3, 4)) + "\n"
    lines = subprocess.run([programs[which]], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    expected = {"accepted": 1, "accepted_noisy": 1, "step_of_one_cell": 1}
    for k, (name, f, tau) in enumerate(cases):
        got = lines[k].split()
        assert got[0] == "refine", lines[k]
        x, y, t0, dx, dy, cov, refined = locate_ref.refine(f, tau, 1e5 + k, 7.0 + k, 3 + k, 20 - k, GRID)
        want = np.array([x, y, t0, dx, dy, cov[0], cov[1], cov[2]], dtype=np.float64)
        have = np.array([unhx(v) for v in got[1:9]])
        assert np.array_equal(have, want, equal_nan=True), (name, have, want)
        assert int(got[9]) == refined == expected.get(name, 0), name
        if not refined:
            assert dx == 0.0 and dy == 0.0 and np.isnan(cov).all()
            assert x == GRID[0] + (3 + k) * GRID[1] and y == GRID[3] + (20 - k) * GRID[4] and t0 == (1e5 + k) + tau[1, 1]
    # an exact quadratic is found exactly, up to rounding: the minimum of "accepted" is at (0.31, -0.22) cells
    x, y, _, dx, dy, cov, _ = locate_ref.refine(cases[0][1], cases[0][2], 0.0, 7.0, 3, 20, GRID)
    assert abs(dx - 0.31) < 1e-12 and abs(dy + 0.22) < 1e-12
    H = np.array([[2.0, 0.4], [0.4, 1.4]])                   # the Hessian of 1.0 x^2 + 2 0.2 x y + 0.7 y^2
    S = np.diag([GRID[1], GRID[4]])
    want = (2.0 / 7.0) * S @ np.linalg.inv(H) @ S
    assert np.allclose([cov[0], cov[1], cov[2]], [want[0, 0], want[0, 1], want[1, 1]], rtol=1e-10, atol=0.0)


@pytest.mark.parametrize("which", ["plain", "san"])
def test_node_program_agrees_with_the_restatement_bit_for_bit(programs, which):
    """the two passes of one node: picks offset by 1e5 s, holes in the table, weights that drop picks, a need nobody meets"""
    rng = np.random.default_rng(5)
    cases, text = [], ""
    for k in range(24):
        P = (1, 2, 7, 33)[k % 4]
        t = 1e5 + rng.uniform(0.0, 3.0, P)
        T = rng.uniform(0.0, 3.0, P)
        T[rng.random(P) < 0.2] = np.nan
        t[rng.random(P) < 0.15] = np.nan
        w = None
        if k % 3:
            w = rng.uniform(0.5, 2.0, P)
            w[rng.random(P) < 0.2] = (0.0, -1.0, np.nan, np.inf)[k % 4]
        need = None if k % 5 else P - 1
        valid = np.isfinite(t) & (np.ones(P, dtype=bool) if w is None else np.isfinite(w) & (w > 0))
        ref = t[np.flatnonzero(valid)[0]] if valid.any() else np.nan
        tr = np.where(valid, t - ref, np.nan)
        nd = int(valid.sum()) if need is None else need
        text += f"node {P} {int(w is not None)} {nd}\n" + "".join(f"{hx(tr[r])} {hx(0.0 if w is None or not valid[r] else w[r])} {hx(T[r])}\n" for r in range(P))
        cases.append((T, t, w, need))
    lines = subprocess.run([programs[which]], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    some_candidate = some_not = False
    for k, (T, t, w, need) in enumerate(cases):
        ref, n, sw, tau, obj, cand = locate_ref.event_maps(T.reshape(-1, 1, 1), t, w, need)
        got = lines[k].split()
        assert got[0] == "node" and int(got[1]) == int(n[0, 0]), (k, lines[k])
        have = np.array([unhx(v) for v in got[2:5]])
        # no valid pick: the program's sums are the empty ones, where the restatement has NaN
        want = np.array([sw[0, 0] if ref is not None else 0.0, tau[0, 0], obj[0, 0]])
        assert np.array_equal(have, want, equal_nan=True), (k, have, want)
        some_candidate |= bool(cand[0, 0])
        some_not |= not cand[0, 0]
    assert some_candidate and some_not


# ---------------------------------------------------------------- the restatement against truth
def closed_form(seed=0, E=200):
    """a constant medium n = 1.5: T = n hypot; 7 stations in two wells left and right of a 37 x 29 grid of spacing 0.1"""
    n, h = 1.5, 0.1
    grid = (-2.0, h, 37, -2.3, h, 29)
    sy = np.linspace(-2.6, 0.9, 7)
    sx = np.where(np.arange(7) % 2 == 0, -2.4, 2.1)
    X, Y = grid[0] + h * np.arange(37), grid[3] + h * np.arange(29)
    T = np.stack([n * np.hypot(X[None, :] - sx[k], Y[:, None] - sy[k]) for k in range(7)])
    rng = np.random.default_rng(seed)
    ev = np.c_[rng.uniform(-1.7, 1.3, E), rng.uniform(-2.0, 0.2, E)]
    t = 3.0 + n * np.hypot(ev[:, 0:1] - sx[None, :], ev[:, 1:2] - sy[None, :])
    return grid, T, ev, t, n, h


def test_restatement_finds_the_truth_on_closed_form_tables():
    grid, T, ev, t, n, h = closed_form()
    o = locate_ref.locate(T, t, grid=grid)
    cx, cy = (ev[:, 0] - grid[0]) / h, (ev[:, 1] - grid[3]) / h
    node_err = max(np.abs(o["ix"] - cx).max(), np.abs(o["iy"] - cy).max())
    loc_err = max(np.abs(o["x"] - ev[:, 0]).max(), np.abs(o["y"] - ev[:, 1]).max()) / h
    t0_err, t0_node_err = np.abs(o["t0_refined"] - 3.0).max(), np.abs(o["t0"] - 3.0).max()
    print(f"best node {node_err:.3f} cell, refined {loc_err:.4f} cell, t0 refined {t0_err:.2e} s, t0 at the node {t0_node_err:.2e} s")
    assert o["refined"].all()                                # every event of this set refines
    assert (o["count"] == 7).all() and np.array_equal(o["sw"], np.full(len(ev), 7.0))
    assert node_err <= 1.0
    assert loc_err <= 0.1
    assert t0_err < n * h / 10
    # the covariance is that of a minimum: positive definite
    assert (o["cov"][:, 0] > 0).all() and (o["cov"][:, 0] * o["cov"][:, 2] - o["cov"][:, 1] ** 2 > 0).all()
    # the window is the map's 3 x 3 slice and the node is the map's first minimum
    for e in (0, 17, 199):
        ix, iy = o["ix"][e], o["iy"][e]
        assert np.array_equal(o["win_obj"][e], o["maps"][e][iy - 1:iy + 2, ix - 1:ix + 2])
        assert o["node"][e] == np.argmin(o["maps"][e])


def test_restatement_rules():
    grid, T, ev, t, n, h = closed_form(E=6)
    # ties go to the least node index: one station, two nodes at the same distance; no weights is weights of 1 here (1 d = d)
    T1 = T[:1].copy()
    t1 = t[:1, :1]
    o = locate_ref.locate(T1, t1)
    assert o["obj"][0] == 0.0 and o["node"][0] == 0          # one pick: every node fits it exactly; node 0 is the least
    a, b = locate_ref.locate(T, t), locate_ref.locate(T, t, w=np.ones_like(t))
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    # no valid pick, and a need that no node meets: node -1 and NaN
    tt = t.copy()
    tt[1] = np.nan
    o = locate_ref.locate(T, tt, need=np.array([7, 7, 8, 7, 7, 7]))
    for e in (1, 2):
        assert o["node"][e] == o["ix"][e] == o["iy"][e] == -1 and o["count"][e] == 0
        assert all(np.isnan(o[k][e]).all() for k in ("sw", "obj", "t0", "ref", "win_obj", "win_tau"))
        assert np.isinf(o["maps"][e]).all()
    assert (o["node"][[0, 3, 4, 5]] >= 0).all()
    # a best node on the rim: NaN outside the grid, no refinement
    Tc = T.copy()
    ev0 = np.array([[grid[0], grid[3] + 5 * h]])
    sx, sy = np.where(np.arange(7) % 2 == 0, -2.4, 2.1), np.linspace(-2.6, 0.9, 7)
    t0 = 1.0 + n * np.hypot(ev0[:, 0:1] - sx[None, :], ev0[:, 1:2] - sy[None, :])
    o = locate_ref.locate(Tc, t0, grid=grid)
    assert o["ix"][0] == 0 and o["iy"][0] == 5 and np.isnan(o["win_obj"][0][:, 0]).all() and np.isfinite(o["win_obj"][0][:, 1:]).all()
    assert o["refined"][0] == 0 and o["x"][0] == grid[0] and np.isnan(o["cov"][0]).all()
