"""CPU: the source-factored scheme of the eikonal fill (rtmi_eikonal_params.scheme).  The field sits where
reserved0 sat, the structs keep their sizes and the ABI version stays 7; a scheme that is neither plain nor factored is refused by
both fills and by rtmi_eikonal_tomo_create before any device work, naming the field; rt_eikonal.h as a program of its own
(tests/native/eikonal_factored.cpp, plain and under the sanitizers) agrees with tests/eikonal_factored_ref.py bit for bit on the
corrected update's branches -- a parent on either side on each axis, a or b +inf, the one-sided ties, d < 0, gdx != gdy, a source
on a grid line, a node on the source, an obstacle's n_src -- and on whole solves.  What needs a device is in
tests/test_gpu_eikonal_factored.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import eikonal_factored_ref as F
import eikonal_ref as R
from conftest import ROOT
from raytracing_amd import _lib, rt_bench

INF = math.inf


# ---------------------------------------------------------------------------------------------------------- the C ABI
def test_the_field_sits_where_reserved0_sat(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include "rtmi.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %d %d %d\\n", '
                   'sizeof(rtmi_eikonal_params), offsetof(rtmi_eikonal_params, max_rounds), offsetof(rtmi_eikonal_params, scheme), '
                   'offsetof(rtmi_eikonal_params, reserved), RTMI_EIKONAL_PLAIN, RTMI_EIKONAL_FACTORED, RTMI_ABI_VERSION); '
                   'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    P = _lib.EikonalParams
    assert got == [C.sizeof(P), P.max_rounds.offset, P.scheme.offset, P.reserved.offset, _lib.EIKONAL_PLAIN, _lib.EIKONAL_FACTORED, 7]
    assert got[:4] == [96, 56, 60, 64] and got[4:6] == [0, 1]          # the layout of the struct that had reserved0 there
    assert not hasattr(P, "reserved0") and _lib.lib().rtmi_abi_version() == 7
    assert rt_bench.eikonal_params((0.0, 0.5, 4, 0.0, 0.25, 3)).scheme == 0
    assert rt_bench.eikonal_params((0.0, 0.5, 4, 0.0, 0.25, 3), scheme="factored").scheme == 1


def params(**kw):
    ep = rt_bench.eikonal_params((0.0, 0.5, 4, 0.0, 0.25, 3))
    for k, v in kw.items():
        setattr(ep, k, v)
    return ep


@pytest.mark.parametrize("scheme", [2, -1])
def test_an_unknown_scheme_is_refused_before_any_device_work(scheme):
    L = _lib.lib()
    n = np.ones((3, 4)); src = np.array([[0.1, 0.1]]); ns = np.ones(1); rec = np.array([[0.5, 0.25], [1.0, 0.3]])
    ep = params(scheme=scheme)
    assert L.rtmi_eikonal_fill(C.byref(ep), _lib.dptr(n), 1, _lib.dptr(src), _lib.dptr(ns), None, None, None, None) == -1
    msg = L.rtmi_last_error().decode()
    assert "rtmi_eikonal_fill:" in msg and "scheme" in msg
    # the device form's pointers are never read: the refusal comes first
    assert L.rtmi_eikonal_fill_dev(C.byref(ep), n.ctypes.data, 1, src.ctypes.data, ns.ctypes.data, None, None, None, None) == -1
    msg = L.rtmi_last_error().decode()
    assert "rtmi_eikonal_fill_dev:" in msg and "scheme" in msg
    h = C.c_void_p(0x1234)
    assert L.rtmi_eikonal_tomo_create(C.byref(ep), _lib.dptr(n), 1, _lib.dptr(src), _lib.dptr(ns), None, None, 2, _lib.dptr(rec),
                                      C.byref(h)) == -1
    msg = L.rtmi_last_error().decode()
    assert "rtmi_eikonal_tomo_create:" in msg and "scheme" in msg and h.value is None
    # and with no source at all both values that exist are no work
    for ok in (0, 1):
        st = _lib.EikonalStats()
        assert L.rtmi_eikonal_fill(C.byref(params(scheme=ok)), None, 0, None, None, None, None, None, C.byref(st)) == 0
    assert L.rtmi_eikonal_fill(C.byref(ep), None, 0, None, None, None, None, None, None) == -1


def test_python_layer_refuses_bad_schemes():
    g = (0.0, 0.5, 4, 0.0, 0.25, 3)
    n = np.ones((3, 4))
    with pytest.raises(ValueError, match="scheme"):
        rt_bench.eikonal_fill(n, [[0.0, 0.0]], g, n_src=[1.0], scheme="fast")
    with pytest.raises(ValueError, match="scheme"):
        rt_bench.eikonal_fill(n, [[0.0, 0.0]], g, n_src=[1.0], scheme=1)
    with pytest.raises(ValueError, match="scheme"):
        rt_bench.EikonalTomography(n, [[0.1, 0.1]], g, [[0.5, 0.25]], n_src=[1.0], scheme="fast")
    fill = {"T": np.ones((1, 3, 4)), "filled": np.ones((1, 3, 4), dtype=np.uint8)}
    for scheme in ("plain", "factored"):
        with pytest.raises(ValueError, match="fill_result"):
            rt_bench.EikonalTomography(n, [[0.1, 0.1]], g, [[0.5, 0.25]], n_src=[1.0], fill_result=fill, scheme=scheme)
    with pytest.raises(ValueError, match="fill_scheme"):
        rt_bench.traveltime_table(None, None, [[0.0, 0.0]], g, thetas=[0.0], step=0.1, max_size=2, box=(0, 1, 0, 1), fill="eikonal",
                                  fill_scheme="fast")


def test_no_not_covered_list_names_the_factored_scheme_any_more():
    import re
    src = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    for m in re.finditer(r"Not covered:(.*?)\*/", src, flags=re.S):
        assert "factored" not in m.group(1).lower()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for m in re.finditer(r"\*\*Not covered\.\*\*(.*?)\n\n", design, flags=re.S):
        if "factored" in m.group(1).lower():                 # section 39's own list: what of the factored scheme is missing
            assert "linearisation of the factored update" in m.group(1)


# ---------------------------------------------------------------------------------------------- rt_eikonal.h as a program
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("eikonal_factored")
    src = os.path.join(ROOT, "tests", "native", "eikonal_factored.cpp")
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


def step(v, k):
    """v moved by k units in the last place"""
    for _ in range(abs(k)):
        v = math.nextafter(v, INF if k > 0 else -INF)
    return v


def reading_for(target, guess, corrected):
    """a raw reading near `guess` whose corrected value (corrected(raw)) is `target` to the bit, or None: the correction is two
    rounded additions, so not every target has one"""
    for k in range(0, 65):
        for raw in (step(guess, k), step(guess, -k)):
            if corrected(raw) == target:
                return raw
    return None


G = (-1.0, 0.3, 17, 0.5, 0.7, 11)             # gdx != gdy
NODE = (6, 4)                                 # X = 0.8, Y = 3.3
#          xs, ys: north-east, south-west, north-west and south-east of the node, and on its grid lines
AROUND = [(1.234, 3.71), (0.31, 2.9), (0.31, 3.71), (1.234, 2.9), (-1.0 + 6.0 * 0.3, 2.2), (0.1, 0.5 + 4.0 * 0.7)]


def update_cases():
    """(grid, i, j, xs, ys, n_src, l, r, dn, up, s) and the branches they were built for"""
    cases, tags = [], []
    i, j = NODE
    s, ns = 0.9, 1.1
    for (xs, ys) in AROUND:
        for l, r in ((1.0, 1.2), (1.2, 1.0), (INF, 1.0), (1.0, INF), (INF, INF), (1.0, 1.0)):
            for dn, up in ((1.1, 1.3), (1.3, 1.1), (INF, 1.1), (1.1, INF), (INF, INF), (1.1, 1.1)):
                cases.append((G, i, j, xs, ys, ns, l, r, dn, up, s))
                tags.append(("east" if r < l else "west", "north" if up < dn else "south"))
    # the one-sided ties ta == b and tb == a, on the corrected readings
    ties = 0
    for (xs, ys) in AROUND[:4]:
        a, b = F.readings(G, i, j, xs, ys, ns, 1.0, INF, 1.1, INF)
        ta, tb = a + G[1] * s, b + G[4] * s
        dn = reading_for(ta, 1.1 + (ta - b), lambda raw: F.readings(G, i, j, xs, ys, ns, 1.0, INF, raw, INF)[1])
        if dn is not None:
            cases.append((G, i, j, xs, ys, ns, 1.0, INF, dn, INF, s)); tags.append("ta == b"); ties += 1
        l = reading_for(tb, 1.0 + (tb - a), lambda raw: F.readings(G, i, j, xs, ys, ns, raw, INF, 1.1, INF)[0])
        if l is not None:
            cases.append((G, i, j, xs, ys, ns, l, INF, 1.1, INF, s)); tags.append("tb == a"); ties += 1
    # a node on the source (rr == 0) and an obstacle's n_src: the plain update, whatever the readings
    for ns_ in (ns, 0.0, -1.0, math.nan, INF):
        cases.append((G, i, j, -1.0 + 6.0 * 0.3, 0.5 + 4.0 * 0.7, ns_, 1.0, 1.2, 1.3, 1.1, s)); tags.append("left out")
        cases.append((G, i, j, 0.31, 2.9, ns_, 1.0, 1.2, 1.3, 1.1, s)); tags.append("left out" if R.obstacle(ns_) else "factored")
    return cases, tags, ties


# d < 0 inside the two-sided branch is a matter of rounding alone, and rare (tests/test_eikonal_host.py): its case, reached through
# the corrected readings by raw readings found to the bit
D_NEGATIVE = tuple(float.fromhex(v) for v in ("0x1.91d6772bd3b77p-1", "0x1.af78523f160c4p-31", "0x1.a6cb32d63f530p-4",
                                              "0x1.8b7348581aeedp+0", "0x1.d631527f1206ep+0"))


def d_negative_case():
    gdx, gdy, a, b, s = D_NEGATIVE
    g = (0.0, gdx, 9, 0.0, gdy, 9)
    i, j, xs, ys, ns = 4, 4, 1.0, 3.0 * gdy + 0.25 * gdy, 1.0
    l = reading_for(a, a + (F.readings(g, i, j, xs, ys, ns, a, INF, INF, INF)[0] - a) * -1.0,
                    lambda raw: F.readings(g, i, j, xs, ys, ns, raw, INF, INF, INF)[0])
    dn = reading_for(b, b + (F.readings(g, i, j, xs, ys, ns, INF, INF, b, INF)[1] - b) * -1.0,
                     lambda raw: F.readings(g, i, j, xs, ys, ns, INF, INF, raw, INF)[1])
    return None if l is None or dn is None else (g, i, j, xs, ys, ns, l, INF, dn, INF, s)


def test_the_cases_take_the_branches_they_were_built_for():
    cases, tags, ties = update_cases()
    assert {t for t in tags if isinstance(t, tuple)} == {("east", "north"), ("east", "south"), ("west", "north"), ("west", "south")}
    assert ties >= 2 and {"ta == b", "tb == a"} <= set(tags)
    for c, tag in zip(cases, tags):
        g, i, j, xs, ys, ns, l, r, dn, up, s = c
        a, b = F.readings(g, i, j, xs, ys, ns, l, r, dn, up)
        raw = (r if r < l else l, up if up < dn else dn)
        if tag == "ta == b":
            assert a + g[1] * s == b
        elif tag == "tb == a":
            assert b + g[4] * s == a
        elif tag == "left out":
            assert (a, b) == raw
        elif tag == "factored":
            assert a != raw[0] and b != raw[1]
    # a source on the node's grid line: dx == 0 and px is a zero, so a is the reading plus T0's difference alone
    g, i, j, xs, ys, ns, l, r, dn, up, s = next(c for c in cases if c[3] == AROUND[4][0] and c[6:8] == (1.0, 1.2))
    T0x, dx, _, rr = F.t0(g, i, j, xs, ys, ns)
    assert dx == 0.0 and rr > 0.0 and F.readings(g, i, j, xs, ys, ns, l, r, dn, up)[0] == l + (T0x - F.t0(g, i - 1, j, xs, ys, ns)[0])
    dneg = d_negative_case()
    assert dneg is not None
    g, i, j, xs, ys, ns, l, r, dn, up, s = dneg
    a, b = F.readings(g, i, j, xs, ys, ns, l, r, dn, up)
    assert (a, b) == D_NEGATIVE[2:4] and (a, b) != (l, dn)
    ta, tb, e = a + g[1] * s, b + g[4] * s, a - b
    wx, wy = 1.0 / (g[1] * g[1]), 1.0 / (g[4] * g[4])
    assert ta > b and tb > a and (wx + wy) * (s * s) - (wx * wy) * (e * e) < 0.0
    assert F.update(*dneg) == min(ta, tb)


@pytest.mark.parametrize("which", ["plain", "san"])
def test_corrected_update_matches_the_restatement(programs, which):
    cases = update_cases()[0] + [d_negative_case()]
    rng = np.random.default_rng(39)
    for _ in range(300):
        gdx, gdy = rng.uniform(0.05, 2.0, 2)
        g = (rng.uniform(-3.0, 3.0), gdx, 40, rng.uniform(-3.0, 3.0), gdy, 30)
        i, j = int(rng.integers(1, 39)), int(rng.integers(1, 29))
        xs, ys = g[0] + rng.uniform(-2.0, 41.0) * gdx, g[3] + rng.uniform(-2.0, 31.0) * gdy
        s, ns = rng.uniform(0.01, 3.0, 2)
        t = ns * math.hypot(g[0] + i * gdx - xs, g[3] + j * gdy - ys)
        read = lambda h: INF if rng.random() < 0.1 else max(0.0, t + rng.uniform(-1.2, 1.2) * h * s)          # noqa: E731
        cases.append((g, i, j, xs, ys, ns, read(gdx), read(gdx), read(gdy), read(gdy), s))
    text = "".join("update {} {} {} {} {} {} ".format(hx(g[0]), hx(g[1]), hx(g[3]), hx(g[4]), i, j) + " ".join(hx(v) for v in rest) + "\n"
                   for (g, i, j, *rest) in cases)
    out = run(programs[which], text)
    differ = 0
    for c, line in zip(cases, out):
        want = F.update(*c)
        assert bits(float.fromhex(line.split()[1])) == bits(want), c
        g, i, j, xs, ys, ns, l, r, dn, up, s = c
        differ += want != R.update(g[1], g[4], R.fmin(l, r), R.fmin(dn, up), s)
    assert differ > 300                                  # the correction is no rounding matter: most cases move


def solve_text(scheme, g, n, xs, ys, n_src, ball, max_rounds, T):
    head = "solve {} {} {} {} {} {} {} {} {} {} {} {} {}\n".format(scheme, g[2], g[5], hx(g[0]), hx(g[1]), hx(g[3]), hx(g[4]), hx(xs),
                                                                  hx(ys), hx(n_src), hx(ball), max_rounds, 0 if T is None else 1)
    body = " ".join(hx(v) for v in np.asarray(n).reshape(-1)) + "\n"
    if T is not None:
        body += " ".join(hx(v) for v in np.asarray(T).reshape(-1)) + "\n"
    return head + body


@pytest.mark.parametrize("which", ["plain", "san"])
def test_whole_solves_match_the_restatement(programs, which):
    jobs = []
    n, (ix, iy) = R.winding_corridor()
    g = (0.0, 1.0, 31, 0.0, 1.0, 27)
    T = np.full(n.shape, np.nan)
    jobs.append((1, g, n, ix + 0.25, iy - 0.125, 1.0, 2.0, 0, T))
    jobs.append((1, g, n, ix + 0.25, iy - 0.125, 1.0, 2.0, 1, T))
    jobs.append((0, g, n, ix + 0.25, iy - 0.125, 1.0, 2.0, 0, T))
    g2 = (-2.0, 7.0 / 19, 20, -2.5, 3.5 / 16, 17)                     # the gradient medium on 20 x 17
    X, Y, n2 = F.gradient_medium(g2)
    n2 = n2.copy()
    n2[9, 4:8] = 0.0; n2[3, 12] = np.nan
    xs, ys = F.SOURCES[1]
    T2 = np.where((X - 3.0) ** 2 + (Y + 1.0) ** 2 <= 0.8, R.gradient_truth(X, Y, xs, ys), np.nan)
    T2[0, 0], T2[16, 19] = np.inf, -np.inf
    ns = 1.0 / (18.0 + 2.0 * ys)
    jobs.append((1, g2, n2, xs, ys, ns, 2.0, 0, T2))
    jobs.append((1, g2, n2, xs, ys, ns, 2.0, 0, np.full(n2.shape, np.nan)))
    jobs.append((1, g2, n2, g2[0] + 7 * g2[1], g2[3] + 5 * g2[4], ns, 0.0, 0, np.full(n2.shape, np.nan)))    # a source on a node
    jobs.append((1, g2, n2, xs, ys, 0.0, 2.0, 0, T2))                                                      # an obstacle's n_src
    jobs.append((1, g2, n2, 99.0, ys, ns, 2.0, 0, None))
    out = run(programs[which], "".join(solve_text(*j) for j in jobs))
    k = 0
    for (scheme, g, n, xs, ys, n_src, ball, max_rounds, T) in jobs:
        want, rounds, clean, filled, changes = F.solve_one(g, n, xs, ys, n_src, T=T, ball=ball, max_rounds=max_rounds, scheme=scheme)
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
    # the factored corridor and gradient solves are no copies of the plain ones
    assert not R.same_bits(F.solve_one(jobs[0][1], jobs[0][2], *jobs[0][3:6])[0], R.solve_one(jobs[0][1], jobs[0][2], *jobs[0][3:6])[0])
