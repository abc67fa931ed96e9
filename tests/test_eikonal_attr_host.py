"""CPU: launch angle, direction and spreading at eikonal-filled nodes (rtmi_eikonal_attributes and its _dev form; DESIGN.md
section 38).  The entries are declared, exported and bound and the ABI version stays 7; every refusal comes before any device
work and names the argument; rt_eikonal_attr.h as a program of its own (tests/native/eikonal_attr.cpp, plain and under the
sanitizers) agrees with tests/eikonal_attr_ref.py bit for bit on wrap at +-pi and beside, the two-parent, one-parent and
no-parent gathers, every neighbour pattern of the difference, m == 0, the ball, the direction, and on whole solves, the corridor
under a cap among them.  What needs a device is in tests/test_gpu_eikonal_attr.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import eikonal_attr_ref as A
import eikonal_lin_ref as L
from conftest import ROOT
from raytracing_amd import _lib, rt_bench
from test_eikonal_host import REFUSALS, params

ENTRIES = ["rtmi_eikonal_attributes", "rtmi_eikonal_attributes_dev"]


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
    # after S: src, n_src, T, filled, theta0, then dir, J and G, which may be null
    tail = [ptr(src), ptr(ns), ptr(tab), ptr(filled), ptr(out), None, None, None]
    for word, kw in REFUSALS:
        assert fn(C.byref(params(**kw)), ptr(n), 1, *tail, None, None) == -1, kw
        msg = lib.rtmi_last_error().decode()
        assert entry + ":" in msg and word in msg, (kw, msg)
    assert fn(C.byref(params()), ptr(n), -1, *tail, None, None) == -1 and "S must be >= 0" in lib.rtmi_last_error().decode()
    for k, name in enumerate(("null src", "null n_src", "null T", "null filled", "null theta0")):
        args = list(tail)
        args[k] = None
        assert fn(C.byref(params()), ptr(n), 1, *args, None, None) == -1
        assert name in lib.rtmi_last_error().decode(), (name, lib.rtmi_last_error())
    assert fn(C.byref(params()), None, 1, *tail, None, None) == -1 and "null n" in lib.rtmi_last_error().decode()
    assert fn(None, ptr(n), 1, *tail, None, None) == -1
    ep = params()
    ep.reserved[0] = 2
    assert fn(C.byref(ep), ptr(n), 1, *tail, None, None) == -1 and "reserved[0]" in lib.rtmi_last_error().decode()


def test_no_sources_is_no_work():
    st = _lib.EikonalStats()
    assert _lib.lib().rtmi_eikonal_attributes(C.byref(params()), None, 0, *[None] * 8, None, C.byref(st)) == 0
    assert (st.free_nodes, st.filled, st.changes, st.rounds_max) == (0, 0, 0, 0)


def test_python_layer_refuses_bad_shapes():
    g = (0.0, 0.5, 4, 0.0, 0.25, 3)
    T, filled = np.ones((1, 3, 4)), np.ones((1, 3, 4), dtype=np.uint8)
    with pytest.raises(ValueError, match="n_src"):
        rt_bench.eikonal_attributes(np.ones((3, 4)), [[0.0, 0.0]], g, T, filled)
    with pytest.raises(ValueError, match="n must be"):
        rt_bench.eikonal_attributes(np.ones((4, 3)), [[0.0, 0.0]], g, T, filled, n_src=[1.0])
    with pytest.raises(ValueError, match="T and filled"):
        rt_bench.eikonal_attributes(np.ones((3, 4)), [[0.0, 0.0]], g, np.ones((2, 3, 4)), filled, n_src=[1.0])
    for name in ("theta0", "theta", "J", "G"):
        with pytest.raises(ValueError, match=f"{name} must be"):
            rt_bench.eikonal_attributes(np.ones((3, 4)), [[0.0, 0.0]], g, T, filled, n_src=[1.0], **{name: np.ones((3, 4))})
    with pytest.raises(ValueError, match="fill_attributes needs"):
        rt_bench.traveltime_table(None, None, [[0.0, 0.0]], g, thetas=[0.0, 0.1], step=0.1, max_size=1.0, box=None, fill_attributes=True)


# ------------------------------------------------------------------------------------------ rt_eikonal_attr.h as a program
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("eikonal_attr")
    src = os.path.join(ROOT, "tests", "native", "eikonal_attr.cpp")
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


def got(line, name):
    w = line.split()
    assert w[0] == name, line
    return [float.fromhex(v) for v in w[1:]]


def same(a, b):
    """the same bits, or both NaN (a NaN's sign and payload are the processor's)"""
    return (math.isnan(a) and math.isnan(b)) or L.bits(a) == L.bits(b)


PI = math.pi
BESIDE = [PI, math.nextafter(PI, 4.0), math.nextafter(PI, 0.0), 2.0 * PI, 3.0, 6.0, 0.0, 1e-300, math.inf, math.nan]
ANGLES = [0.0, 0.5, -0.5, 3.0, -3.0, 3.1, -3.1, PI, -PI, 6.2, math.nan, math.inf, -math.inf]


@pytest.mark.parametrize("which", ["plain", "san"])
def test_the_pieces_match_the_restatement(programs, which):
    jobs = []                                           # (the command's line, its name, what the restatement gives)
    for d in BESIDE:
        for v in (d, -d):
            jobs.append((f"wrap {hx(v)}", "wrap", [A.wrap(v)]))
    for par, ca, cb in ((5, 0.25, 0.75), (5, 0.5, 0.25), (7, 1e-3, 0.999), (1, 1.0, 0.0), (4, 0.0, 1.0), (0, 0.0, 0.0), (5, 0.0, 0.0)):
        jobs.append((f"weight {par} {hx(ca)} {hx(cb)}", "weight", [A.weight(par, ca, cb)]))
    for ha in (0, 1):
        for hb in (0, 1):
            for ta in ANGLES:
                for tb in ANGLES:
                    for w in (0.25, 1.0 / 3.0):
                        jobs.append((f"combine {ha} {hx(ta)} {hb} {hx(tb)} {hx(w)}", "combine", [A.combine(bool(ha), ta, bool(hb), tb, w)]))
    finite = [a for a in ANGLES if math.isfinite(a)]
    for ul in (0, 1):
        for uh in (0, 1):
            for lo in finite:
                for hi in finite:
                    jobs.append((f"diff {ul} {hx(lo)} {hx(0.7)} {uh} {hx(hi)} {hx(0.125)}", "diff",
                                 [A.diff(bool(ul), lo, 0.7, bool(uh), hi, 0.125)]))
    for ddx, ddy, s in ((0.0, 0.0, 0.5), (3.0, 4.0, 0.5), (1e-200, 0.0, 2.0), (0.3, -0.1, 1.0 / 18.0), (1e200, 1e200, 1.0)):
        J = A.spread(ddx, ddy)
        jobs.append((f"spread {hx(ddx)} {hx(ddy)} {hx(s)}", "spread", [J, A.amp(s, J)]))
    for par in range(16):
        for t, a, b in ((2.0, 1.0, 1.5), (2.0, 2.0, 1.5), (2.0, 2.0, 2.0), (1.0 / 3.0, 0.1, 0.3)):
            jobs.append((f"dir {hx(0.3)} {hx(0.7)} {par} {hx(t)} {hx(a)} {hx(b)}", "dir", list(A.free_dir(0.3, 0.7, par, t, a, b))))
    g = (-2.0, 0.1, 9, -2.5, 0.0625, 9)
    for i, j, xs, ys in ((3, 4, -2.0 + 3.0 * 0.1, -2.25), (3, 4, -1.71, -2.23), (0, 0, -1.6, -2.2), (8, 8, -1.3, -1.9), (2, 7, -1.65, -2.3)):
        X, Y = g[0] + float(i) * g[1], g[3] + float(j) * g[4]
        dx, dy = X - xs, Y - ys
        r = math.sqrt(dx * dx + dy * dy)
        jobs.append((f"ball {hx(g[0])} {hx(g[1])} {hx(g[3])} {hx(g[4])} {i} {j} {hx(xs)} {hx(ys)} {hx(0.5)}", "ball",
                     [math.atan2(dy, dx), *A.ball_dir(dx, dy, r), r, A.amp(0.5, r)]))
    out = run(programs[which], "".join(j[0] + "\n" for j in jobs))
    assert len(jobs) > 1500
    for (line, name, want), o in zip(jobs, out):
        have = got(o, name)
        assert len(have) == len(want) and all(same(a, b) for a, b in zip(have, want)), (line, have, want)
    # the cases that were meant are there: the source node itself, wrap firing in a gather and in a difference, m == 0
    assert jobs[-5][2][1:4] == [0.0, 0.0, 0.0] and A.amp(0.5, 0.0) == math.inf
    assert A.combine(True, 3.1, True, -3.1, 0.25) > 3.1 and A.diff(True, 3.1, 0.7, True, -3.1, 0.125) > 0.0


def solve_text(grid, n, xs, ys, n_src, ball, max_rounds, T, filled, arrays):
    head = "solve {} {} {} {} {} {} {} {} {} {} {}\n".format(grid[2], grid[5], hx(grid[0]), hx(grid[1]), hx(grid[3]), hx(grid[4]),
                                                           hx(xs), hx(ys), hx(n_src), hx(ball), max_rounds)
    return head + words(n) + "\n" + words(T) + "\n" + " ".join(str(int(v)) for v in filled.reshape(-1)) + "\n" + \
        "".join(words(a) + "\n" for a in arrays)


@pytest.mark.parametrize("which", ["plain", "san"])
def test_whole_solves_match_the_restatement(programs, which):
    jobs = []
    for name, max_rounds in (("corridor_case", 0), ("corridor_case", 1), ("walls_case", 0), ("disc_case", 0)):
        grid, n, src, ns, fill, nets = L.filled(getattr(L, name)())
        s = len(src) - 1
        rng = np.random.default_rng(37)
        ins = [rng.uniform(-3.1, 3.1, n.shape)] + [rng.standard_normal(n.shape) for _ in range(4)]
        if name == "walls_case":                        # seeds that cannot be used
            seeds = np.flatnonzero(np.array(nets[s].cls) == L.SEED)
            ins[0].reshape(-1)[seeds[:3]] = (np.nan, np.inf, -np.inf)
        jobs.append((grid, n, src[s], ns[s], fill["T"][s], fill["filled"][s], nets[s], max_rounds, ins))
    text = "".join(solve_text(grid, n, xy[0], xy[1], n_src, 2.0, mr, T, filled, ins) for grid, n, xy, n_src, T, filled, _, mr, ins in jobs)
    out = run(programs[which], text)
    for k, (grid, n, xy, n_src, T, filled, net, mr, ins) in enumerate(jobs):
        want = A.solve_one(grid, n, xy[0], xy[1], n_src, T, filled, *ins, max_rounds=mr, net=net)
        lines = out[6 * k:6 * k + 6]
        assert lines[0].split() == ["solve", str(want["rounds"]), str(want["clean"]), str(len(net.free) + net.cls.count(L.BALL)),
                                    str(want["changes"])]
        for key, line in zip(A.KEYS, lines[1:]):
            assert L.same_but_nan(np.array(got(line, key)).reshape(n.shape), want[key]), (k, key)
        # dead nodes and seeds keep the bits of every array
        keep = np.array(net.cls).reshape(n.shape) <= L.SEED
        for key, a in zip(A.KEYS, ins):
            assert L.same_but_nan(want[key][keep], a[keep]) and (keep.any() or k < 2)       # the corridor has neither
    grid, n, xy, n_src, T, filled, net, mr, ins = jobs[1]
    assert mr == 1 and A.solve_one(grid, n, xy[0], xy[1], n_src, T, filled, max_rounds=1, net=net)["clean"] == 0
