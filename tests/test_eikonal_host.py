"""CPU: the eikonal continuation of traveltime tables (rtmi_eikonal_fill, rtmi_eikonal_fill_dev).  The
entries are declared, exported and bound with the header's signatures, the structs have gcc's sizes and the ABI version stays 7;
every refusal comes before any device work and names the argument; rt_eikonal.h as a program of its own
(tests/native/eikonal_update.cpp, plain and under the sanitizers) agrees with tests/eikonal_ref.py bit for bit on the update's
branches -- a or b +inf, the ties ta == b and tb == a, d < 0, gdx != gdy, a denormal e --, on the states and the ball, and on
whole solves.  What needs a device is in tests/test_gpu_eikonal.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import eikonal_ref as R
from conftest import ROOT
from raytracing_amd import _lib, rt_bench


# ---------------------------------------------------------------------------------------------------------- the C ABI
def test_structs_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include "rtmi.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %zu\\n", '
                   'sizeof(rtmi_eikonal_params), sizeof(rtmi_eikonal_stats), offsetof(rtmi_eikonal_params, ball), '
                   'offsetof(rtmi_eikonal_params, reserved), offsetof(rtmi_eikonal_stats, kernel_ms)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert sizes == [C.sizeof(_lib.EikonalParams), C.sizeof(_lib.EikonalStats), _lib.EikonalParams.ball.offset,
                     _lib.EikonalParams.reserved.offset, _lib.EikonalStats.kernel_ms.offset]
    assert _lib.lib().rtmi_abi_version() == 7
    assert {"rtmi_eikonal_fill", "rtmi_eikonal_fill_dev"} <= set(_lib.SYMBOLS)


def params(**kw):
    ep = rt_bench.eikonal_params((0.0, 0.5, 4, 0.0, 0.25, 3))
    for k, v in kw.items():
        setattr(ep, k, v)
    return ep


REFUSALS = [("nx", dict(nx=0)), ("ny", dict(ny=0)), ("ny", dict(ny=-3)), ("2^31", dict(nx=1 << 16, ny=(1 << 15) + 1)),
            ("gdx", dict(gdx=0.0)), ("gdx", dict(gdx=-1.0)), ("gdy", dict(gdy=math.inf)), ("gdy", dict(gdy=math.nan)),
            ("max_rounds", dict(max_rounds=-1)), ("ball", dict(ball=math.inf)), ("ball", dict(ball=math.nan))]


@pytest.mark.parametrize("entry", ["rtmi_eikonal_fill", "rtmi_eikonal_fill_dev"])
def test_argument_errors_come_before_any_device_work(entry):
    L = _lib.lib()
    fn = getattr(L, entry)
    n = np.ones((3, 4)); src = np.zeros((1, 2)); ns = np.ones(1)
    host = entry == "rtmi_eikonal_fill"
    ptr = (lambda a: _lib.dptr(a)) if host else (lambda a: a.ctypes.data)      # never read: the refusal comes first
    for word, kw in REFUSALS:
        assert fn(C.byref(params(**kw)), ptr(n), 1, ptr(src), ptr(ns), None, None, None, None) == -1, kw
        msg = L.rtmi_last_error().decode()
        assert entry + ":" in msg and word in msg, (kw, msg)
    assert fn(C.byref(params()), ptr(n), -1, ptr(src), ptr(ns), None, None, None, None) == -1
    assert "S must be >= 0" in L.rtmi_last_error().decode()
    for k, name in enumerate(("null n", "null src", "null n_src")):
        args = [ptr(n), 1, ptr(src), ptr(ns)]
        args[(0, 2, 3)[k]] = None
        assert fn(C.byref(params()), *args, None, None, None, None) == -1
        assert name in L.rtmi_last_error().decode()
    assert fn(None, ptr(n), 1, ptr(src), ptr(ns), None, None, None, None) == -1
    # nx ny == 2^31 itself is not refused for its size: the next refusal in line answers
    assert fn(C.byref(params(nx=1 << 16, ny=1 << 15, max_rounds=-1)), ptr(n), 1, ptr(src), ptr(ns), None, None, None, None) == -1
    assert "max_rounds" in L.rtmi_last_error().decode()


def test_no_sources_is_no_work():
    st = _lib.EikonalStats()
    assert _lib.lib().rtmi_eikonal_fill(C.byref(params()), None, 0, None, None, None, None, None, C.byref(st)) == 0
    assert (st.free_nodes, st.filled, st.unreached, st.rounds_max) == (0, 0, 0, 0)


def test_python_layer_refuses_bad_shapes():
    g = (0.0, 0.5, 4, 0.0, 0.25, 3)
    with pytest.raises(ValueError, match="n_src"):
        rt_bench.eikonal_fill(np.ones((3, 4)), [[0.0, 0.0]], g)
    with pytest.raises(ValueError, match="n must be"):
        rt_bench.eikonal_fill(np.ones((4, 3)), [[0.0, 0.0]], g, n_src=[1.0])
    with pytest.raises(ValueError, match="T must be"):
        rt_bench.eikonal_fill(np.ones((3, 4)), [[0.0, 0.0]], g, np.zeros((2, 3, 4)), n_src=[1.0])
    with pytest.raises(ValueError, match="n_src must be"):
        rt_bench.eikonal_fill(np.ones((3, 4)), [[0.0, 0.0]], g, n_src=[1.0, 2.0])
    with pytest.raises(_lib.RtmiError, match="ball"):
        rt_bench.eikonal_fill(np.ones((3, 4)), [[0.0, 0.0]], g, n_src=[1.0], ball=math.nan)


# ---------------------------------------------------------------------------------------------- rt_eikonal.h as a program
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("eikonal_update")
    src = os.path.join(ROOT, "tests", "native", "eikonal_update.cpp")
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


def bits(v):
    return np.float64(v).view(np.uint64)


DENORMAL = 5e-324
#            gdx, gdy, a, b, s
UPDATES = [(0.5, 0.25, math.inf, math.inf, 1.0),           # both +inf: no change
           (0.5, 0.25, 1.0, math.inf, 2.0), (0.5, 0.25, math.inf, 1.0, 2.0),       # a or b +inf
           (0.5, 0.25, 1.0, 2.0, 2.0), (0.5, 0.25, 1.5, 1.0, 2.0),                 # the ties ta == b and tb == a
           (0.5, 0.25, 1.0, 1.0 + 0.49, 2.0), (0.5, 0.25, 1.0 + 0.2, 1.0, 2.0),    # two-sided, gdx != gdy
           (0.1, 0.1, 1.0, 1.0 + 2.0 ** -52, 3.0),                             # e of one ulp
           (0.1, 0.1, DENORMAL, 0.0, 3.0), (0.1, 0.3, 0.0, DENORMAL, 1e-3),        # a denormal e
           (1e-3, 1e3, 7.0, 7.0 + 1e-4, 0.5), (1e3, 1e-3, 7.0 + 1e-4, 7.0, 0.5),   # spacings six decades apart
           (0.3, 0.7, 1.0, 1.2, 1.0 / 3.0), (0.3, 0.7, 2.0, 1.9, 1.0 / 3.0),
           (0.5, 0.5, 1.0, 1.0, 1e-200), (0.5, 0.5, 1e300, 1e300, 1e300)]           # s s underflows; everything overflows


# d < 0 inside the two-sided branch is a matter of rounding alone (ta > b and tb > a bound |e| below the larger step), and rare:
# one case in 20 000 drawn near the tie with spacings nine decades apart.  This is that case.
D_NEGATIVE = tuple(float.fromhex(v) for v in ("0x1.91d6772bd3b77p-1", "0x1.af78523f160c4p-31", "0x1.a6cb32d63f530p-4",
                                              "0x1.8b7348581aeedp+0", "0x1.d631527f1206ep+0"))


def test_the_d_negative_case_takes_that_branch():
    gdx, gdy, a, b, s = D_NEGATIVE
    ta, tb = a + gdx * s, b + gdy * s
    wx, wy = 1.0 / (gdx * gdx), 1.0 / (gdy * gdy)
    e = a - b
    assert ta > b and tb > a and (wx + wy) * (s * s) - (wx * wy) * (e * e) < 0.0
    assert R.update(*D_NEGATIVE) == min(ta, tb)


@pytest.mark.parametrize("which", ["plain", "san"])
def test_update_and_states_match_the_restatement(programs, which):
    cases = list(UPDATES) + [D_NEGATIVE]
    rng = np.random.default_rng(3)
    for _ in range(300):
        gdx, gdy = rng.uniform(0.05, 2.0, 2)
        a = rng.uniform(0.0, 5.0)
        s = rng.uniform(0.01, 3.0)
        cases.append((gdx, gdy, a, a + rng.uniform(-1.2, 1.2) * min(gdx, gdy) * s, s))
    text = "".join("update " + " ".join(hx(v) for v in c) + "\n" for c in cases)
    out = run(programs[which], text)
    for c, line in zip(cases, out):
        assert bits(float.fromhex(line.split()[1])) == bits(R.update(*c)), c
    # the states and the ball
    g = (-1.0, 0.5, 9, 2.0, 0.25, 7)
    inits = []
    for s, tin in ((1.0, math.nan), (1.0, 3.5), (1.0, -0.0), (1.0, math.inf), (1.0, -math.inf), (0.0, 3.5), (-1.0, math.nan),
                   (math.nan, 1.0), (math.inf, math.nan)):
        for ball, n_src in ((2.0, 1.25), (-1.0, 1.25), (0.0, 1.25), (2.0, math.nan), (2.0, 0.0), (1e3, 0.75)):
            for (i, j, xs, ys) in ((3, 2, 0.5, 2.5), (3, 2, 0.61, 2.43), (0, 0, -7.0, 9.0), (4, 4, 1.0 + 2.0 * 0.5, 3.0)):
                inits.append((g, i, j, s, tin, xs, ys, n_src, ball))
    text = "".join("init {} {} {} {} {} {} ".format(hx(g[0]), hx(g[1]), hx(g[3]), hx(g[4]), i, j) +
                   " ".join(hx(v) for v in (s, tin, xs, ys, n_src, ball)) + "\n" for (g, i, j, s, tin, xs, ys, n_src, ball) in inits)
    out = run(programs[which], text)
    states = set()
    for c, line in zip(inits, out):
        st, w = R.init(*c)
        states.add(st)
        assert int(line.split()[1]) == st and bits(float.fromhex(line.split()[2])) == bits(w), c
    assert states == {R.FROZEN, R.FREE, R.BALL}


def solve_text(g, n, xs, ys, n_src, ball, max_rounds, T):
    head = "solve {} {} {} {} {} {} {} {} {} {} {} {}\n".format(g[2], g[5], hx(g[0]), hx(g[1]), hx(g[3]), hx(g[4]), hx(xs), hx(ys),
                                                               hx(n_src), hx(ball), max_rounds, 0 if T is None else 1)
    body = " ".join(hx(v) for v in np.asarray(n).reshape(-1)) + "\n"
    if T is not None:
        body += " ".join(hx(v) for v in np.asarray(T).reshape(-1)) + "\n"
    return head + body


@pytest.mark.parametrize("which", ["plain", "san"])
def test_whole_solves_match_the_restatement(programs, which):
    rng = np.random.default_rng(17)
    jobs = []
    n, (ix, iy) = R.winding_corridor()
    g = (0.0, 1.0, 31, 0.0, 1.0, 27)
    T = np.full(n.shape, np.nan)
    jobs.append((g, n, ix + 0.25, iy - 0.125, 1.0, 2.0, 0, T))
    jobs.append((g, n, ix + 0.25, iy - 0.125, 1.0, 2.0, 1, T))
    g2 = (-1.0, 0.3, 17, 0.5, 0.7, 11)
    n2 = rng.uniform(0.2, 3.0, (11, 17))
    n2[4, 5:9] = 0.0; n2[2, 2] = np.nan
    T2 = np.where(rng.random(n2.shape) < 0.2, rng.uniform(0.0, 4.0, n2.shape), np.nan)
    T2[0, 0], T2[10, 16], T2[4, 6] = np.inf, -np.inf, 2.0
    jobs.append((g2, n2, 1.234, 3.21, 0.9, 2.0, 0, T2))
    jobs.append((g2, n2, 1.234, 3.21, 0.9, -1.0, 0, T2))
    jobs.append((g2, n2, 99.0, 3.21, 0.9, 2.0, 0, None))
    out = run(programs[which], "".join(solve_text(*j) for j in jobs))
    k = 0
    for (g, n, xs, ys, n_src, ball, max_rounds, T) in jobs:
        want, rounds, clean, filled, changes = R.solve_one(g, n, xs, ys, n_src, T=T, ball=ball, max_rounds=max_rounds)
        head = out[k].split()
        assert head[0] == "solve" and [int(v) for v in head[1:3]] == [rounds, clean]
        assert int(head[4]) == int(filled.sum()) and int(head[5]) == changes
        k += 1
        if T is not None:
            got = np.array([float.fromhex(v) for v in out[k].split()[1:]]).reshape(want.shape)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan) and R.same_bits(np.where(nan, 0.0, got), np.where(nan, 0.0, want))
            k += 1
        assert out[k].split()[1] == "".join(str(int(v)) for v in filled.reshape(-1))
        k += 1
