"""CPU: first-arrival eikonal tomography on the device (rtmi_eikonal_tomo_*).  The entries are declared,
exported and bound and the ABI version stays 7; every refusal of the handle's arguments comes before any device work and names the
argument; rt_eikonal_tomo.h as a program of its own (tests/native/eikonal_tomo.cpp, plain and under the sanitizers) agrees with
tests/eikonal_tomo_ref.py bit for bit on the cell weights, the samples, the spread lists (offsets and order) and the live-row
rule.  What needs a device is in tests/test_gpu_eikonal_tomo.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import eikonal_lin_ref as L
import eikonal_tomo_ref as E
from conftest import ROOT
from raytracing_amd import _lib, rt_bench
from test_eikonal_host import REFUSALS, params

ENTRIES = {"rtmi_eikonal_tomo_create": 10, "rtmi_eikonal_tomo_destroy": 1, "rtmi_eikonal_tomo_info": 3, "rtmi_eikonal_tomo_table": 4,
           "rtmi_eikonal_tomo_apply": 4, "rtmi_eikonal_tomo_apply_dev": 4, "rtmi_eikonal_tomo_transpose": 4,
           "rtmi_eikonal_tomo_transpose_dev": 4, "rtmi_eikonal_tomo_residual": 3, "rtmi_eikonal_tomo_residual_dev": 3,
           "rtmi_eikonal_tomo_relinearise": 3, "rtmi_eikonal_tomo_relinearise_dev": 3, "rtmi_eikonal_tomo_lsqr": 8}


def test_entries_are_bound_and_the_abi_version_stays():
    assert set(ENTRIES) <= set(_lib.SYMBOLS) and _lib.lib().rtmi_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    for e, nargs in ENTRIES.items():
        assert f" {e}(" in header and len(_lib.SYMBOLS[e][1]) == nargs
    assert "#define RTMI_ABI_VERSION 7" in header and C.sizeof(_lib.EikonalTomoStats) == 8 * 8 + 4 * 4 + 2 * 8 + 4 * 8


def create(ep, n, S, src, ns, T, filled, R, rec):
    h = C.c_void_p(0x1234)
    u8 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))        # noqa: E731
    rc = _lib.lib().rtmi_eikonal_tomo_create(C.byref(ep) if ep is not None else None, _lib.dptr(n), S, _lib.dptr(src), _lib.dptr(ns),
                                             _lib.dptr(T), u8(filled), R, _lib.dptr(rec), C.byref(h))
    return rc, h.value, _lib.lib().rtmi_last_error().decode()


def test_argument_errors_come_before_any_device_work():
    n = np.ones((3, 4)); src = np.array([[0.1, 0.1]]); ns = np.ones(1); rec = np.array([[0.5, 0.25], [1.5, 0.5]])
    tab = np.ones((1, 3, 4)); filled = np.ones((1, 3, 4), dtype=np.uint8)
    for word, kw in REFUSALS:                                         # everything rtmi_eikonal_fill refuses
        rc, h, msg = create(params(**kw), n, 1, src, ns, None, None, 2, rec)
        assert rc == -1 and h is None and "rtmi_eikonal_tomo_create:" in msg and word in msg, (kw, msg)
    ep = params()
    g = (ep.gx0, ep.gdx, ep.nx, ep.gy0, ep.gdy, ep.ny)
    inside = np.array([E.at(g, 0.5, 0.5), E.at(g, 1.0, 1.0)])
    for args, word in (((ep, n, 0, src, ns, None, None, 2, inside), "S must be >= 1"),
                       ((ep, n, 1, src, ns, None, None, 0, inside), "R must be >= 1"),
                       ((ep, n, 1, src, ns, None, None, 2, None), "null rec"),
                       ((ep, n, 1, src, ns, tab, None, 2, inside), "exactly one of T and filled is null"),
                       ((ep, n, 1, src, ns, None, filled, 2, inside), "exactly one of T and filled is null"),
                       ((ep, None, 1, src, ns, None, None, 2, inside), "null n"),
                       ((None, n, 1, src, ns, None, None, 2, inside), "null ep")):
        rc, h, msg = create(*args)
        assert rc == -1 and h is None and word in msg, (word, msg)
    far = float(ep.gx0 + (ep.nx - 1) * ep.gdx)
    for bad in ([np.nan, inside[0, 1]], [inside[0, 0], np.inf], [ep.gx0 - 1e-9, inside[0, 1]], [np.nextafter(far, np.inf), inside[0, 1]],
                [inside[0, 0], ep.gy0 + ep.ny * ep.gdy]):
        rc, h, msg = create(ep, n, 1, src, ns, None, None, 2, np.array([inside[0], bad]))
        assert rc == -1 and h is None and "receiver 1 is not finite or lies outside the grid" in msg, (bad, msg)
    lib = _lib.lib()
    for entry in ("rtmi_eikonal_tomo_apply", "rtmi_eikonal_tomo_transpose", "rtmi_eikonal_tomo_apply_dev", "rtmi_eikonal_tomo_transpose_dev"):
        assert getattr(lib, entry)(None, None, None, None) == -1 and "null handle" in lib.rtmi_last_error().decode()
    assert lib.rtmi_eikonal_tomo_lsqr(None, None, None, None, None, None, None, None) == -1
    lib.rtmi_eikonal_tomo_destroy(None)


def test_python_layer_refuses_bad_shapes():
    g = (0.0, 0.5, 4, 0.0, 0.25, 3)
    with pytest.raises(ValueError, match="n_src"):
        rt_bench.EikonalTomography(np.ones((3, 4)), [[0.0, 0.0]], g, [[0.5, 0.25]])
    with pytest.raises(ValueError, match="n must be"):
        rt_bench.EikonalTomography(np.ones((4, 3)), [[0.0, 0.0]], g, [[0.5, 0.25]], n_src=[1.0])
    with pytest.raises(ValueError, match="fill_result"):
        rt_bench.EikonalTomography(np.ones((3, 4)), [[0.0, 0.0]], g, [[0.5, 0.25]], n_src=[1.0],
                                   fill_result={"T": np.ones((2, 3, 4)), "filled": np.ones((1, 3, 4), dtype=np.uint8)})
    with pytest.raises(_lib.RtmiError, match="receiver 0"):
        rt_bench.EikonalTomography(np.ones((3, 4)), [[0.0, 0.0]], g, [[1.75, 0.25]], n_src=[1.0])


# ------------------------------------------------------------------------------------------ rt_eikonal_tomo.h as a program
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("eikonal_tomo")
    src = os.path.join(ROOT, "tests", "native", "eikonal_tomo.cpp")
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


def points(grid, rng, count):
    """points on nodes, on edges, in cells, on the last column and row, outside, and not finite"""
    gx0, gdx, nx, gy0, gdy, ny = grid
    pts = [E.at(grid, u, v) for u in (0.0, 1.0, 1.5, nx - 2.0, nx - 1.5, nx - 1.0) for v in (0.0, 0.5, 2.0, ny - 1.25, ny - 1.0)]
    pts += [[gx0 - 0.3 * gdx, gy0], [gx0, gy0 + (ny + 2) * gdy], [np.nan, gy0], [gx0, np.inf], [-np.inf, gy0], [gx0 + 1e300, gy0]]
    pts += [[gx0 + u * gdx, gy0 + v * gdy] for u, v in rng.uniform(-1.0, 1.0, (count, 2)) * [nx + 1, ny + 1]]
    return np.array(pts)


@pytest.mark.parametrize("which", ["plain", "san"])
def test_cells_and_samples_match_the_restatement(programs, which):
    rng = np.random.default_rng(12)
    cases = []
    for grid in (L.GRADIENT_GRID, (0.5, 0.25, 1, -1.0, 0.2, 9), (0.5, 0.25, 9, -1.0, 0.2, 1), (0.0, 1.0, 1, 0.0, 1.0, 1), (-3.0, 0.1, 2, 7.0, 0.3, 2)):
        for x, y in points(grid, rng, 40):
            for source in (0, 1):
                cases.append((grid, x, y, source))
    text = "".join("cell {} {} {} {} {} {} {} {} {}\n".format(g[2], g[5], hx(g[0]), hx(g[1]), hx(g[3]), hx(g[4]), hx(x), hx(y), s)
                   for g, x, y, s in cases)
    out = run(programs[which], text)
    zero = 0
    for (g, x, y, s), line in zip(cases, out):
        idx, w, inside = E.cell(g, x, y, bool(s))
        f = line.split()
        assert f[0] == "cell" and int(f[1]) == int(inside) and int(f[2]) == int(E.receiver_ok(g, x, y)), (g, x, y, s, line)
        assert [int(v) for v in f[3:7]] == idx and [L.bits(float.fromhex(v)) for v in f[7:11]] == [L.bits(v) for v in w], (g, x, y, s, line)
        assert all(0 <= i < g[2] * g[5] for i in idx)
        zero += s and not inside
        if s and not inside:
            assert w == [0.0] * 4 and idx[0] == 0 and not any(np.signbit(w))
    assert zero > 50
    vals = rng.standard_normal((200, 8)) * np.exp(rng.uniform(-30, 30, (200, 1)))
    out = run(programs[which], "".join("sample " + " ".join(hx(v) for v in row) + "\n" for row in vals))
    for row, line in zip(vals, out):
        assert L.bits(float.fromhex(line.split()[1])) == L.bits(E.sample(row[4:], [0, 1, 2, 3], row[:4]))


@pytest.mark.parametrize("which", ["plain", "san"])
def test_lists_and_live_rows_match_the_restatement(programs, which):
    jobs = []
    for name in ("13x11", "1x9", "9x1"):
        op = E.shape_case(name)[5]
        jobs += [(op.ridx, None), (op.sidx, op.inside)]
    grid, n, src, ns, fill, rec, wop = E.walls()
    jobs += [(wop.ridx, None), (wop.sidx, wop.inside), (np.zeros((0, 4), dtype=np.int64), None)]
    text = ""
    for idx, take in jobs:
        text += f"lists {len(idx)} {int(take is not None)}\n" + " ".join(str(int(v)) for v in idx.reshape(-1)) + "\n"
        if take is not None:
            text += " ".join(str(int(v)) for v in take) + "\n"
    for s in range(len(src)):
        text += f"live {n.size} {len(rec)}\n" + " ".join(hx(v) for v in n.reshape(-1)) + "\n" + \
            " ".join(hx(v) for v in fill["T"][s].reshape(-1)) + "\n" + " ".join(str(int(v)) for v in wop.ridx.reshape(-1)) + "\n"
    out = run(programs[which], text)
    k = 0
    shared = 0
    for idx, take in jobs:
        node, off, pair = E.lists(idx, take)
        for name, want in (("node", node), ("off", off), ("pair", pair)):
            f = out[k].split()
            assert f[0] == name and [int(v) for v in f[1:]] == list(want), (name, out[k])
            k += 1
        assert list(node) == sorted(set(node)) and off[0] == 0 and off[-1] == len(pair)
        for q in range(len(node)):
            seg = pair[off[q]:off[q + 1]]
            assert list(seg) == sorted(seg) and all(idx.reshape(-1)[p] == node[q] for p in seg)
            shared += len({p >> 2 for p in seg}) > 1
    assert shared > 0                                                 # two receivers in one cell share nodes
    for s in range(len(src)):
        f = out[k].split()
        assert f[0] == "live" and [int(v) for v in f[1:]] == [int(v) for v in wop.live[s]]
        k += 1
    assert (~wop.live).any() and wop.live.any()
