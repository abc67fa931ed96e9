"""CPU: pick-free detection and location by stacking station traces (rtmi_locate_stack, rtmi_locate_stack_dev; DESIGN.md section
30).  The entries are declared, exported and bound with the header's signatures, the structs have gcc's sizes and offsets and the
ABI version stays 7; the refusals that need no device come before any device work and name the argument; rt_stack.h as a program
of its own (tests/native/stack_events.cpp, plain and under the sanitizers) agrees with tests/stack_ref.py bit for bit on the event
selection and on both refinements; the restatement finds planted events on closed-form tables.  What needs a handle is in
tests/test_gpu_stack.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import stack_ref
from conftest import ROOT
from raytracing_amd import _lib, rt_bench

_dp = C.POINTER(C.c_double)
NAMES = ("rtmi_locate_stack", "rtmi_locate_stack_dev")


def _prototype(name, ret="int"):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtmi.h")).read(), flags=re.S)
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entries():
    assert _prototype("rtmi_locate_stack") == [
        "rtmi_locator *loc", "const rtmi_stack_params *sp", "const double *c", "const double *w", "double *peak", "int32_t *peak_node",
        "double *best", "int32_t *best_m", "double *volume", "rtmi_stack_event *events", "int64_t *nev", "rtmi_stack_stats *st"]
    assert _prototype("rtmi_locate_stack_dev") == [
        "rtmi_locator *loc", "const rtmi_stack_params *sp", "const double *d_c", "const double *d_w", "double *d_peak",
        "int32_t *d_peak_node", "double *d_best", "int32_t *d_best_m", "double *d_volume", "rtmi_stack_event *events", "int64_t *nev",
        "rtmi_stack_stats *st"]
    src = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert re.search(r"#define\s+RTMI_ABI_VERSION\s+7\b", src)


def test_ctypes_signatures_and_exports():
    sp, ev, st, n = C.POINTER(_lib.StackParams), C.POINTER(_lib.StackEvent), C.POINTER(_lib.StackStats), C.POINTER(C.c_int64)
    ip, vp = _lib._ip, C.c_void_p
    assert _lib.SYMBOLS["rtmi_locate_stack"] == (C.c_int, [vp, sp, _dp, _dp, _dp, ip, _dp, ip, _dp, ev, n, st])
    assert _lib.SYMBOLS["rtmi_locate_stack_dev"] == (C.c_int, [vp, sp, vp, vp, vp, vp, vp, vp, vp, ev, n, st])
    _lib.lib()                                                                # first: it maps the HIP runtime the library shares with torch
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name)
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    assert _lib.lib().rtmi_abi_version() == 7 and _lib.ABI_VERSION == 7
    for name in ("stack", "stack_device"):
        assert callable(getattr(rt_bench.Locator, name))


def test_struct_sizes_and_offsets_match_gccs(tmp_path):
    fields = {"rtmi_stack_params": ("nt", "M", "ct0", "cdt", "o0", "od", "need", "threshold", "min_sep", "max_events", "reserved"),
              "rtmi_stack_event": ("m", "node", "ix", "iy", "n", "value", "t0", "win", "x", "y", "t0_refined", "dx", "dy", "dm", "refined",
                                   "reserved"),
              "rtmi_stack_stats": ("kernel_ms", "upload_ms", "triples", "contributing", "truncated", "reserved")}
    types = {"rtmi_stack_params": _lib.StackParams, "rtmi_stack_event": _lib.StackEvent, "rtmi_stack_stats": _lib.StackStats}
    body = "".join(f'printf("%zu\\n", sizeof({t}));' + "".join(f'printf("%zu\\n", offsetof({t}, {f}));' for f in fs) for t, fs in fields.items())
    src = tmp_path / "sz.c"
    src.write_text('#include "rtmi.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){' + body + 'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = []
    for t, fs in fields.items():
        want += [C.sizeof(types[t])] + [getattr(types[t], f).offset for f in fs]
    assert got == want


# ---------------------------------------------------------------- refusals without a device
FAKE = C.c_void_p(8)              # never dereferenced: the checks below come before the handle is read
BUF = (C.c_double * 8)()
IBUF = (C.c_int32 * 8)()


def _refused(rc, who, *words):
    msg = _lib.lib().rtmi_last_error()
    assert rc == -1, msg
    assert msg.startswith(who.encode() + b": "), msg
    for w in words:
        assert w.encode() in msg, msg


def _params(**kw):
    sp = _lib.StackParams()
    sp.nt, sp.M, sp.ct0, sp.cdt, sp.o0, sp.od, sp.need, sp.threshold, sp.min_sep, sp.max_events = 8, 4, 0.0, 0.01, 0.0, 0.01, 0, 0.5, 0, 0
    for k, v in kw.items():
        setattr(sp, k, v)
    return sp


@pytest.mark.parametrize("name", NAMES)
def test_refusals_that_need_no_device(name):
    fn = getattr(_lib.lib(), name)
    dev = name.endswith("_dev")
    d, i = (C.c_void_p(64), C.c_void_p(128)) if dev else (BUF, IBUF)
    ev = (_lib.StackEvent * 2)()
    nev = C.c_int64(0)

    def call(loc=FAKE, sp=None, c=d, peak=d, peak_node=i, events=ev, n=nev, null_sp=False):
        sp = _params() if sp is None else sp
        return fn(loc, None if null_sp else C.byref(sp), c, None, peak, peak_node, None, None, None, events,
                  None if n is None else C.byref(n), None)

    _refused(call(loc=None), name, "null handle")
    _refused(call(null_sp=True), name, "null sp")
    _refused(call(c=None), name, "null c")
    _refused(call(peak=None), name, "null peak")
    _refused(call(peak_node=None), name, "null peak_node")
    _refused(call(n=None), name, "null nev")
    _refused(call(sp=_params(max_events=1), events=None), name, "null events with max_events > 0")
    for nt in (1, 0, -4):
        _refused(call(sp=_params(nt=nt)), name, "nt must be >= 2")
    _refused(call(sp=_params(nt=2 ** 31 + 1)), name, "nt is over 2^31")
    for M in (0, -1):
        _refused(call(sp=_params(M=M)), name, "M must be >= 1")
    for bad in (0.0, -0.01, float("nan"), float("inf")):
        _refused(call(sp=_params(cdt=bad)), name, "cdt must be finite and > 0")
        _refused(call(sp=_params(od=bad)), name, "od must be finite and > 0")
    for bad in (float("nan"), float("inf"), -float("inf")):
        _refused(call(sp=_params(ct0=bad)), name, "ct0 must be finite")
        _refused(call(sp=_params(o0=bad)), name, "o0 must be finite")
    _refused(call(sp=_params(need=-1)), name, "need is negative")
    _refused(call(sp=_params(min_sep=-1)), name, "min_sep is negative")
    _refused(call(sp=_params(max_events=-1), events=None), name, "max_events is negative")
    _refused(call(sp=_params(threshold=float("nan"))), name, "threshold is NaN")
    for M in (2 ** 31 - 16, 2 ** 40):                        # the limit of the scan's own length needs no handle either
        _refused(call(sp=_params(M=M)), name, "M is over 2^31 - 17", "2^31 (tile of 256 nodes, chunk of 16 scan indices) pairs")


def test_python_checks_shapes_first():
    class Shape(rt_bench.Locator):
        def __init__(self):
            self.P, self.ny, self.nx, self.grid, self._h = 3, 4, 5, (0.0, 1.0, 5, 0.0, 1.0, 4), None

    S = Shape()
    with pytest.raises(ValueError, match=r"traces must be \[3, nt\]"):
        S.stack(np.zeros((2, 40)), 0.01, scan=(0.0, 0.01, 4))
    with pytest.raises(ValueError, match=r"weights must be \[3\]"):
        S.stack(np.zeros((3, 40)), 0.01, scan=(0.0, 0.01, 4), weights=np.ones(2))
    with pytest.raises(RuntimeError, match="closed"):
        S.stack(np.zeros((3, 40)), 0.01, scan=(0.0, 0.01, 4))
    with pytest.raises(TypeError, match="traces must be a torch tensor"):
        S.stack_device(np.zeros((3, 40)), 0.01, scan=(0.0, 0.01, 4))


# ---------------------------------------------------------------- rt_stack.h as a program
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("stack_events")
    src = os.path.join(ROOT, "tests", "native", "stack_events.cpp")
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


def series():
    """(name, peak, peak_node, threshold, min_sep, max_events)"""
    rng = np.random.default_rng(3)
    M = 40
    p = rng.uniform(0.0, 1.0, M)
    nodes = rng.integers(0, 100, M).astype(np.int32)
    tied = np.round(p * 4) / 4                               # five levels: many ties
    holes = p.copy()
    holes[::3] = -np.inf
    hn = nodes.copy()
    hn[::3] = -1
    hn[7] = -1                                               # a finite peak without a node is not eligible
    out = [("plain", p, nodes, 0.3, 2, 100), ("ties", tied, nodes, 0.25, 1, 100), ("ties_sep_0", tied, nodes, 0.5, 0, 100),
           ("sep_0", p, nodes, 0.5, 0, 100), ("sep_1", p, nodes, 0.0, 1, 100), ("sep_M", p, nodes, 0.0, M, 100),
           ("sep_over_M", p, nodes, 0.0, 10 * M, 100), ("max_events_reached", p, nodes, 0.2, 1, 3), ("max_events_0", p, nodes, 0.2, 1, 0),
           ("max_events_exact", p, nodes, 0.0, M, 1), ("threshold_minus_inf", holes, hn, -np.inf, 3, 100),
           ("threshold_plus_inf", p, nodes, np.inf, 0, 100), ("all_minus_inf", np.full(M, -np.inf), np.full(M, -1, dtype=np.int32), -np.inf, 0, 100),
           ("minus_inf_with_nodes", np.full(M, -np.inf), nodes, -np.inf, 4, 100), ("one_sample", p[:1], nodes[:1], 0.0, 0, 5)]
    return out


@pytest.mark.parametrize("which", ["plain", "san"])
def test_selection_program_agrees_with_the_restatement(programs, which):
    cases = series()
    text = ""
    for _, p, nodes, thr, sep, mx in cases:
        text += f"select {len(p)} {hx(thr)} {sep} {mx}\n" + "".join(f"{hx(a)} {b}\n" for a, b in zip(p, nodes))
    lines = subprocess.run([programs[which]], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    seen = {}
    for k, (name, p, nodes, thr, sep, mx) in enumerate(cases):
        taken, remained = stack_ref.select(p, nodes, thr, sep, mx)
        got = lines[k].split()
        assert got[0] == "select" and int(got[1]) == len(taken) and int(got[2]) == int(remained), (name, lines[k], taken, remained)
        assert [int(v) for v in got[3:]] == taken, name
        seen[name] = (taken, remained)
        # what the rule promises, whatever the implementation: apart by more than min_sep, descending, eligible
        assert all(abs(a - b) > sep for i, a in enumerate(taken) for b in taken[:i])
        assert all(p[a] >= p[b] for a, b in zip(taken, taken[1:])) and all(p[m] >= thr and nodes[m] >= 0 for m in taken)
    assert len(seen["sep_M"][0]) == 1 and len(seen["sep_over_M"][0]) == 1 and not seen["sep_M"][1]
    assert seen["max_events_reached"] == (seen["max_events_reached"][0][:3], True) and len(seen["max_events_reached"][0]) == 3
    assert seen["max_events_0"] == ([], True) and seen["max_events_exact"][1] is False
    assert seen["threshold_plus_inf"] == ([], False) and seen["all_minus_inf"] == ([], False)
    assert len(seen["minus_inf_with_nodes"][0]) == 8 and seen["minus_inf_with_nodes"][0][0] == 0   # all tied: the least m first
    assert 7 not in seen["threshold_minus_inf"][0] and all(m % 3 for m in seen["threshold_minus_inf"][0])
    t = seen["ties_sep_0"][0]
    assert all(a < b for a, b in zip(t, t[1:]) if cases[2][1][a] == cases[2][1][b])              # ties in ascending m


GRID = (-2.0, 0.1, 37, -2.3, 0.125, 29)


def hill(x0, y0, m0, a=1.0, b=0.6, cm=0.8, top=2.0, sign=-1.0):
    d, j, i = np.meshgrid((-1.0, 0.0, 1.0), (-1.0, 0.0, 1.0), (-1.0, 0.0, 1.0), indexing="ij")
    return top + sign * (a * (i - x0) ** 2 + b * (j - y0) ** 2 + cm * (d - m0) ** 2)


def windows():
    rng = np.random.default_rng(17)
    W = {"accepted": hill(0.31, -0.22, 0.4), "accepted_noisy": hill(-0.4, 0.45, -0.3) + 1e-3 * rng.standard_normal((3, 3, 3)),
         "minimum": hill(0.1, 0.1, 0.2, sign=1.0), "time_step_over_one": hill(0.2, 0.1, 1.6), "space_step_over_one": hill(1.7, 0.0, 0.1),
         "time_step_of_one": hill(0.0, 0.0, 1.0, cm=0.5), "flat": np.full((3, 3, 3), 0.25)}
    flat_time = hill(0.2, -0.1, 0.0)
    flat_time[:, 1, 1] = flat_time[1, 1, 1]                  # the three values at the node are equal: the denominator is 0
    W["flat_time"] = flat_time
    for name, at in (("nan_in_space", (1, 2, 0)), ("nan_in_time", (0, 1, 1)), ("nan_elsewhere", (2, 0, 0))):
        w = W["accepted"].copy()
        w[at] = np.nan
        W[name] = w
    inf = W["accepted"].copy()
    inf[2, 1, 1] = -np.inf
    W["minus_inf_in_time"] = inf
    rim = W["accepted"].copy()
    rim[0] = np.nan                                          # an event at scan index 0
    W["first_scan_index"] = rim
    return list(W.items())


EXPECT = {"accepted": 3, "accepted_noisy": 3, "minimum": 0, "time_step_over_one": 1, "space_step_over_one": 2, "time_step_of_one": 3,
          "flat": 0, "flat_time": 1, "nan_in_space": 2, "nan_in_time": 1, "nan_elsewhere": 3, "minus_inf_in_time": 1, "first_scan_index": 1}


@pytest.mark.parametrize("which", ["plain", "san"])
def test_refinement_program_agrees_with_the_restatement_bit_for_bit(programs, which):
    cases = windows()
    text = ""
    for k, (_, w) in enumerate(cases):
        text += "refine " + " ".join(hx(v) for v in w.ravel()) + f" {hx(1e5 + k)} {hx(0.01)} {3 + k} {20 - k} "
        text += " ".join(hx(GRID[q]) for q in (0, 1, 3, 4)) + "\n"
    lines = subprocess.run([programs[which]], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    for k, (name, w) in enumerate(cases):
        got = lines[k].split()
        assert got[0] == "refine", lines[k]
        want = stack_ref.refine(w, 1e5 + k, 0.01, 3 + k, 20 - k, GRID)
        have = np.array([unhx(v) for v in got[1:7]])
        assert np.array_equal(have, np.array(want[:6], dtype=np.float64), equal_nan=True), (name, have, want)
        assert int(got[7]) == want[6] == EXPECT[name], (name, got[7], want[6])
        x, y, t0, dx, dy, dm, refined = want
        if not refined & 1:
            assert dx == 0.0 and dy == 0.0 and x == GRID[0] + (3 + k) * GRID[1] and y == GRID[3] + (20 - k) * GRID[4]
        if not refined & 2:
            assert dm == 0.0 and t0 == 1e5 + k
    # a separable quadratic is found exactly, up to rounding: the top of "accepted" is at (0.31, -0.22) cells and 0.4 scan steps
    x, y, t0, dx, dy, dm, _ = stack_ref.refine(cases[0][1], 50.0, 0.01, 3, 20, GRID)
    assert abs(dx - 0.31) < 1e-12 and abs(dy + 0.22) < 1e-12 and abs(dm - 0.4) < 1e-12 and abs(t0 - 50.004) < 1e-12


# ---------------------------------------------------------------- the restatement against truth
def closed_form(seed=3):
    """A constant medium of slowness 1.5, 7 random stations within one unit of a 37 x 29 grid, three off-grid events: traces of
    Gaussian pulses (sigma 0.08 s) at the true arrival times plus 0.02 |N(0, 1)|"""
    n = 1.5
    grid = (-2.0, 0.1, 37, -2.3, 0.125, 29)
    rng = np.random.default_rng(seed)
    X, Y = grid[0] + grid[1] * np.arange(37), grid[3] + grid[4] * np.arange(29)
    sx, sy = rng.uniform(X[0] - 1.0, X[-1] + 1.0, 7), rng.uniform(Y[0] - 1.0, Y[-1] + 1.0, 7)
    T = n * np.hypot(X[None, None, :] - sx[:, None, None], Y[None, :, None] - sy[:, None, None])
    ev = np.stack([rng.uniform(X[2], X[-3], 3), rng.uniform(Y[2], Y[-3], 3)], axis=1)
    origin = np.array([101.23, 103.117, 104.871])
    nt, cdt, ct0 = 1400, 0.01, 100.0
    tt = ct0 + cdt * np.arange(nt)
    arrive = origin[:, None] + n * np.hypot(ev[:, 0:1] - sx[None, :], ev[:, 1:2] - sy[None, :])          # [event, station]
    c = np.exp(-0.5 * ((tt[None, None, :] - arrive[:, :, None]) / 0.08) ** 2).sum(axis=0) + 0.02 * np.abs(rng.standard_normal((7, nt)))
    return grid, T, c, ev, origin, (ct0, cdt, 100.0, 0.01, 600)


def match(o, ev, origin, grid):
    """per planted event (matched by origin time): node error in cells per axis, refined error in cells, t0 error"""
    assert len(o["m"]) == len(origin)
    order = [int(np.argmin(np.abs(o["t0_node"] - t))) for t in origin]
    assert sorted(order) == list(range(len(origin)))
    k = np.array(order)
    cx, cy = (ev[:, 0] - grid[0]) / grid[1], (ev[:, 1] - grid[3]) / grid[4]
    node = np.maximum(np.abs(o["ix"][k] - cx), np.abs(o["iy"][k] - cy))
    node_d = np.hypot(o["ix"][k] - cx, o["iy"][k] - cy)
    ref_d = np.hypot((o["x"][k] - ev[:, 0]) / grid[1], (o["y"][k] - ev[:, 1]) / grid[4])
    return node, node_d, ref_d, np.abs(o["t0"][k] - origin)


def test_restatement_finds_the_planted_events_on_closed_form_tables():
    grid, T, c, ev, origin, (ct0, cdt, o0, od, M) = closed_form()
    o = stack_ref.stack(T, c, ct0, cdt, o0, od, M, threshold=0.9, min_sep=100, max_events=10, grid=grid)
    assert len(o["m"]) == 3 and not o["truncated"]                       # exactly the planted events
    node, node_d, ref_d, t0_err = match(o, ev, origin, grid)
    print(f"closed form: node {node.max():.3f} cell per axis, distance node {node_d.mean():.3f} / refined {ref_d.mean():.3f} cell "
          f"(mean), refined max {ref_d.max():.3f} cell, t0 {t0_err.max():.4f} s, values {o['value']}")
    assert (node <= 1.0).all()
    assert ref_d.mean() < node_d.mean()
    assert (o["count"] == 7).all() and (o["refined"] == 3).all()
    # the windows are the volume's slices, the projections the volume's
    for k in range(3):
        m, ix, iy = o["m"][k], o["ix"][k], o["iy"][k]
        assert np.array_equal(o["win"][k], o["volume"][m - 1:m + 2, iy - 1:iy + 2, ix - 1:ix + 2])
        assert o["value"][k] == o["peak"][m] == o["volume"][m].max() and o["node"][k] == np.argmax(o["volume"][m])
    assert np.array_equal(o["best"], o["volume"].max(axis=0)) and np.array_equal(o["best_m"], o["volume"].argmax(axis=0))
    # a lower threshold lets noise in: the issue's prototype saw a fourth, spurious event at 0.8; this seed's count is printed
    low = stack_ref.stack(T, c, ct0, cdt, o0, od, M, threshold=0.5, min_sep=100, max_events=10, grid=grid)
    print(f"threshold 0.5: {len(low['m'])} events, values {low['value']}")
    assert list(low["m"][:3]) == list(o["m"])


def test_restatement_rules():
    grid, T, c, ev, origin, (ct0, cdt, o0, od, M) = closed_form()
    M = 40
    o0 = 101.1
    # no weights is weights of 1 (1 v = v exactly, a sum of n ones is n)
    a = stack_ref.stack(T, c, ct0, cdt, o0, od, M, threshold=-np.inf, min_sep=5, max_events=4, grid=grid)
    b = stack_ref.stack(T, c, ct0, cdt, o0, od, M, w=np.ones(7), threshold=-np.inf, min_sep=5, max_events=4, grid=grid)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert len(a["m"]) == 4 and a["truncated"]
    # a weight that drops a station is the station left out of T and c
    w = np.array([1.0, 2.0, 0.0, 0.5, np.nan, 1.5, -1.0])
    keep = np.array([0, 1, 3, 5])
    a = stack_ref.stack(T, c, ct0, cdt, o0, od, M, w=w)
    b = stack_ref.stack(T[keep], c[keep], ct0, cdt, o0, od, M, w=w[keep])
    for k in ("volume", "peak", "peak_node", "best", "best_m", "contributing"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["n"].max() == 4) and np.isfinite(a["peak"]).all()
    # a need nobody meets
    z = stack_ref.stack(T, c, ct0, cdt, o0, od, M, need=8, threshold=-np.inf, max_events=3)
    assert np.isneginf(z["peak"]).all() and (z["peak_node"] == -1).all() and (z["best_m"] == -1).all() and len(z["m"]) == 0
    assert np.isneginf(z["volume"]).all() and not z["truncated"]
    # a scan that runs off the traces: fewer stations contribute, and with need absent those samples are no candidates
    late = stack_ref.stack(T, c, ct0, cdt, 108.0, 0.1, 70)
    assert np.isneginf(late["peak"][-5:]).all() and np.isfinite(late["peak"][:5]).all() and (late["n"][-1] == 0).all()
    some = stack_ref.stack(T, c, ct0, cdt, 108.0, 0.1, 70, need=2)
    assert np.isfinite(some["peak"]).sum() > np.isfinite(late["peak"]).sum()
