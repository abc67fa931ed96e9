"""CPU: the linearised eikonal fill (rtmi_eikonal_tangent, rtmi_eikonal_adjoint and their _dev forms).  The
entries are declared, exported and bound and the ABI version stays 7; every refusal comes before any device work and names the
argument; rt_eikonal_lin.h as a program of its own (tests/native/eikonal_lin.cpp, plain and under the sanitizers) agrees with
tests/eikonal_lin_ref.py bit for bit on the coefficient branches -- one-sided x and y, the ties ta == b and tb == a, west and
south winning theirs, d < 0, gdx != gdy, a dropped parent -- and on whole tangent and adjoint solves.  What needs a device is in
tests/test_gpu_eikonal_lin.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import eikonal_lin_ref as L
import eikonal_ref as R
from conftest import ROOT
from raytracing_amd import _lib, rt_bench
from test_eikonal_host import D_NEGATIVE, REFUSALS, params

ENTRIES = ["rtmi_eikonal_tangent", "rtmi_eikonal_tangent_dev", "rtmi_eikonal_adjoint", "rtmi_eikonal_adjoint_dev"]


def test_entries_are_bound_and_the_abi_version_stays():
    assert set(ENTRIES) <= set(_lib.SYMBOLS) and _lib.lib().rtmi_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    for e in ENTRIES:
        assert f"int {e}(" in header and len(_lib.SYMBOLS[e][1]) == 13


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_come_before_any_device_work(entry):
    lib = _lib.lib()
    fn = getattr(lib, entry)
    n = np.ones((3, 4)); src = np.zeros((1, 2)); ns = np.ones(1); tab = np.ones((1, 3, 4)); filled = np.ones((1, 3, 4), dtype=np.uint8)
    host = not entry.endswith("_dev")
    ptr = (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)) if a.dtype == np.uint8 else _lib.dptr(a)) if host else (lambda a: a.ctypes.data)
    out = np.zeros((1, 3, 4))
    # after S: src, n_src, T, filled, the input, two optional arrays, the output (tangent); ..., r, lam, g, g_src (adjoint)
    tail = [ptr(src), ptr(ns), ptr(tab), ptr(filled), ptr(tab), None, None, ptr(out)] if "tangent" in entry else \
           [ptr(src), ptr(ns), ptr(tab), ptr(filled), ptr(tab), ptr(out), None, None]
    for word, kw in REFUSALS:
        assert fn(C.byref(params(**kw)), ptr(n), 1, *tail, None, None) == -1, kw
        msg = lib.rtmi_last_error().decode()
        assert entry + ":" in msg and word in msg, (kw, msg)
    assert fn(C.byref(params()), ptr(n), -1, *tail, None, None) == -1 and "S must be >= 0" in lib.rtmi_last_error().decode()
    names = ("null src", "null n_src", "null T", "null filled") + (("null dn", None, None, "null dT") if "tangent" in entry
                                                                    else ("null r", "null lam", None, None))
    for k, name in enumerate(names):
        if name is None:
            continue
        args = list(tail)
        args[k] = None
        assert fn(C.byref(params()), ptr(n), 1, *args, None, None) == -1
        assert name in lib.rtmi_last_error().decode(), (name, lib.rtmi_last_error())
    assert fn(C.byref(params()), None, 1, *tail, None, None) == -1 and "null n" in lib.rtmi_last_error().decode()
    assert fn(None, ptr(n), 1, *tail, None, None) == -1


def test_no_sources_is_no_work():
    st = _lib.EikonalStats()
    for entry in ("rtmi_eikonal_tangent", "rtmi_eikonal_adjoint"):
        assert getattr(_lib.lib(), entry)(C.byref(params()), None, 0, *[None] * 8, None, C.byref(st)) == 0
        assert (st.free_nodes, st.filled, st.changes, st.rounds_max) == (0, 0, 0, 0)


def test_python_layer_refuses_bad_shapes():
    g = (0.0, 0.5, 4, 0.0, 0.25, 3)
    fill = {"T": np.ones((1, 3, 4)), "filled": np.ones((1, 3, 4), dtype=np.uint8)}
    with pytest.raises(ValueError, match="n_src"):
        rt_bench.eikonal_tangent(np.ones((3, 4)), [[0.0, 0.0]], g, fill, np.ones((3, 4)))
    with pytest.raises(ValueError, match="n must be"):
        rt_bench.eikonal_tangent(np.ones((4, 3)), [[0.0, 0.0]], g, fill, np.ones((3, 4)), n_src=[1.0])
    with pytest.raises(ValueError, match="dn must be"):
        rt_bench.eikonal_tangent(np.ones((3, 4)), [[0.0, 0.0]], g, fill, np.ones((4, 3)), n_src=[1.0])
    with pytest.raises(ValueError, match="fill_result"):
        rt_bench.eikonal_adjoint(np.ones((3, 4)), [[0.0, 0.0]], g, {"T": np.ones((2, 3, 4)), "filled": fill["filled"]},
                                 np.ones((1, 3, 4)), n_src=[1.0])
    with pytest.raises(ValueError, match="r must be"):
        rt_bench.eikonal_adjoint(np.ones((3, 4)), [[0.0, 0.0]], g, fill, np.ones((3, 4)), n_src=[1.0])
    with pytest.raises(ValueError, match="dT_seed must be"):
        rt_bench.eikonal_tangent(np.ones((3, 4)), [[0.0, 0.0]], g, fill, np.ones((3, 4)), n_src=[1.0], dT_seed=np.ones((3, 4)))


def test_source_weights_are_bilinear_and_zero_outside():
    g = (-1.0, 0.5, 4, 2.0, 0.25, 3)
    idx, w = rt_bench.eikonal_source_weights([[-0.625, 2.3], [0.5, 2.5], [9.0, 2.1], [-1.0, 2.0]], g)
    assert list(idx[0]) == [4, 5, 8, 9] and np.allclose(w[0], [0.25 * 0.8, 0.75 * 0.8, 0.25 * 0.2, 0.75 * 0.2])
    assert list(idx[1]) == [6, 7, 10, 11] and np.allclose(w[1], [0, 0, 0, 1])        # the grid's far corner: the last cell
    assert not w[2].any() and list(w[3]) == [1, 0, 0, 0]
    X, Y = R.nodes(g)
    f = 3.0 + 2.0 * X - 5.0 * Y                                                       # bilinear interpolation is exact on it
    assert np.allclose((f.reshape(-1)[idx] * w).sum(axis=1)[[0, 1, 3]], [3.0 - 1.25 - 11.5, 3.0 + 1.0 - 12.5, 3.0 - 2.0 - 10.0])
    ridx, rw = L.source_weights([[-0.625, 2.3]], g)
    assert np.array_equal(ridx[0], idx[0]) and np.array_equal(rw[0], w[0])


# ------------------------------------------------------------------------------------------ rt_eikonal_lin.h as a program
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("eikonal_lin")
    src = os.path.join(ROOT, "tests", "native", "eikonal_lin.cpp")
    out = {}
    for name, flags in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall"] + flags + ["-o", exe, src])
        out[name] = exe
    return out


def run(exe, text):
    p = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return p.stdout.split("\n")


def hx(v):
    return float(v).hex()


def words(a):
    return " ".join(hx(v) for v in np.asarray(a, dtype=np.float64).reshape(-1))


def values(line, name, shape):
    w = line.split()
    assert w[0] == name
    return np.array([float.fromhex(v) for v in w[1:]]).reshape(shape)


INF = math.inf
#         gdx, gdy, l, r, dn, up, s, t (None: the fill's own update of the node) -> what the case is, (branch, parents)
COEFS = [((0.5, 0.25, 1.0, INF, INF, INF, 2.0, None), "one-sided x, the west parent", L.XPARENT),
         ((0.5, 0.25, 3.0, 1.0, INF, INF, 2.0, None), "one-sided x, the east parent", L.XPARENT | L.XEAST),
         ((0.5, 0.25, INF, INF, 1.0, 4.0, 2.0, None), "one-sided y, the south parent", L.YPARENT),
         ((0.5, 0.25, INF, INF, 4.0, 1.0, 2.0, None), "one-sided y, the north parent", L.YPARENT | L.YNORTH),
         ((0.5, 0.25, 1.0, 5.0, 2.0, 9.0, 2.0, None), "the tie ta == b: one-sided x", L.XPARENT),
         ((0.5, 0.25, 1.5, 5.0, 9.0, 1.0, 2.0, None), "the tie tb == a: one-sided y", L.YPARENT | L.YNORTH),
         ((0.5, 0.25, 1.0, 1.0, 1.25, 1.25, 2.0, None), "l == r and dn == up: west and south win", L.XPARENT | L.YPARENT),
         ((0.5, 0.25, 1.2, 1.0, 1.49, 1.6, 2.0, None), "two-sided, gdx != gdy", L.XPARENT | L.XEAST | L.YPARENT),
         ((0.3, 0.7, 2.0, 2.5, 1.9, INF, 1.0 / 3.0, None), "two-sided", L.XPARENT | L.YPARENT),
         ((0.5, 0.5, 1.0, INF, INF, INF, 1e-20, None), "a + gdx s == a: the parent is dropped", 0),
         ((0.5, 0.25, 1.0, INF, 1.25, INF, 2.0, 1.25), "two-sided with a value at its y-parent's: that parent is dropped", L.XPARENT),
         ((0.5, 0.25, INF, INF, INF, INF, 2.0, 3.0), "no neighbour", 0),
         (D_NEGATIVE[:2] + (D_NEGATIVE[2], INF, D_NEGATIVE[3], INF, D_NEGATIVE[4], None), "d < 0: the smaller one-sided branch", None)]


@pytest.mark.parametrize("which", ["plain", "san"])
def test_coefficients_match_the_restatement(programs, which):
    cases = []
    for c, what, par in COEFS:
        gdx, gdy, l, r, dn, up, s, t = c
        if t is None:
            t = R.update(gdx, gdy, R.fmin(l, r), R.fmin(dn, up), s)
        cases.append(((gdx, gdy, l, r, dn, up, s, t), what, par))
    rng = np.random.default_rng(4)
    for _ in range(300):
        gdx, gdy = rng.uniform(0.05, 2.0, 2)
        a, s = rng.uniform(0.0, 5.0), rng.uniform(0.01, 3.0)
        b = a + rng.uniform(-1.2, 1.2) * min(gdx, gdy) * s
        l, r = (a, a + rng.uniform(0, 1)) if rng.random() < 0.5 else (a + rng.uniform(0, 1), a)
        dn, up = (b, b + rng.uniform(0, 1)) if rng.random() < 0.5 else (b + rng.uniform(0, 1), b)
        cases.append(((gdx, gdy, l, r, dn, up, s, R.update(gdx, gdy, a, b, s)), "a draw", None))
    out = run(programs[which], "".join("coef " + " ".join(hx(v) for v in c) + "\n" for c, _, _ in cases))
    two_sided = 0
    for (c, what, par), line in zip(cases, out):
        ca, cb, cs, p = L.coef(*c)
        w = line.split()
        assert [L.bits(float.fromhex(v)) for v in w[1:4]] == [L.bits(ca), L.bits(cb), L.bits(cs)] and int(w[4]) == p, (what, c)
        assert par is None or p == par, (what, p)
        two_sided += ca != 0.0 and cb != 0.0
    assert two_sided > 100
    # the d < 0 case takes the one-sided branch of the smaller of ta and tb, and the two-sided cases are two-sided
    ca, cb, cs, p = L.coef(*cases[len(COEFS) - 1][0])
    assert (ca, cb) in ((1.0, 0.0), (0.0, 1.0)) and cs in D_NEGATIVE[:2]
    assert all(L.coef(*cases[k][0])[0] not in (0.0, 1.0) for k in (7, 8))
    assert L.coef(*cases[10][0])[1] == 0.0 and L.coef(*cases[10][0])[0] not in (0.0, 1.0)


def solve_text(cmd, grid, n, xs, ys, n_src, ball, max_rounds, T, filled, arrays, extra=""):
    head = "{} {} {} {} {} {} {} {} {} {} {} {}{}\n".format(cmd, grid[2], grid[5], hx(grid[0]), hx(grid[1]), hx(grid[3]), hx(grid[4]),
                                                          hx(xs), hx(ys), hx(n_src), hx(ball), max_rounds, extra)
    return head + words(n) + "\n" + words(T) + "\n" + " ".join(str(int(v)) for v in filled.reshape(-1)) + "\n" + \
        "".join(words(a) + "\n" for a in arrays)


@pytest.mark.parametrize("which", ["plain", "san"])
def test_whole_solves_match_the_restatement(programs, which):
    jobs = []
    for name, max_rounds in (("corridor_case", 0), ("corridor_case", 1), ("walls_case", 0), ("disc_case", 0)):
        grid, n, src, ns, fill, nets = L.filled(getattr(L, name)())
        s = len(src) - 1
        rng = np.random.default_rng(31)
        dn, seed, r = rng.standard_normal(n.shape), rng.standard_normal(n.shape), rng.standard_normal(n.shape)
        jobs.append((grid, n, src[s], ns[s], fill["T"][s], fill["filled"][s], nets[s], max_rounds, dn, 0.375, seed, r))
    text = ""
    for grid, n, xy, n_src, T, filled, net, max_rounds, dn, dn_src, seed, r in jobs:
        text += solve_text("tangent", grid, n, xy[0], xy[1], n_src, 2.0, max_rounds, T, filled, [dn, seed], f" {hx(dn_src)} 1")
        text += solve_text("tangent", grid, n, xy[0], xy[1], n_src, 2.0, max_rounds, T, filled, [dn], f" {hx(dn_src)} 0")
        text += solve_text("adjoint", grid, n, xy[0], xy[1], n_src, 2.0, max_rounds, T, filled, [r])
    out = run(programs[which], text)
    k = 0
    for grid, n, xy, n_src, T, filled, net, max_rounds, dn, dn_src, seed, r in jobs:
        for sd in (seed, None):
            dT, rounds, clean, changes = net.tangent(dn, dn_src, sd, max_rounds=max_rounds)
            assert out[k].split() == ["tangent", str(rounds), str(clean), str(len(net.free) + net.cls.count(L.BALL)), str(changes)]
            assert R.same_bits(values(out[k + 1], "dT", n.shape), dT)
            k += 2
        lam, g, g_src, rounds, clean, changes = net.adjoint(r, max_rounds=max_rounds)
        head = out[k].split()
        assert head[:5] == ["adjoint", str(rounds), str(clean), str(len(net.free) + net.cls.count(L.BALL)), str(changes)]
        assert L.bits(float.fromhex(head[5])) == L.bits(g_src)
        assert R.same_bits(values(out[k + 1], "lam", n.shape), lam) and R.same_bits(values(out[k + 2], "g", n.shape), g)
        k += 3
