"""CPU: the definition of the device's trace filter (include/rtmi.h).  The restatement tests/filter_ref.py
against np.convolve sliced at the origin; the matrix of F^T is the transpose of F's in every bit; the library's half-derivative
taps (rtmi_half_derivative_taps, host only) convolved with themselves are the first difference, and on a cosine they give the
response (1 - exp(-i w dt))^(1/2) / sqrt(dt) within the tail the truncation leaves out; rt_filter.h as a program of its own,
plain and under -fsanitize=address,undefined, against the library's taps and the restatement bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raytracing_amd import rt_bench

import filter_ref as FR

U = 2.0 ** -53


def origins(L):
    return sorted({0, L // 2, L - 1})


def rounding_bound(taps, x):
    """a sum of L products, each rounded, added one at a time: at most L 2^-53 sum|f| max|x| from the exact value"""
    return len(taps) * U * float(np.sum(np.abs(taps))) * float(np.max(np.abs(x)))


@pytest.mark.parametrize("nt", (2, 3, 8, 9, 63, 64, 65, 150, 299, 300))
def test_restatement_equals_numpy_convolve_sliced_at_the_origin(nt):
    rng = np.random.default_rng(nt)
    worst = 0.0
    for L in (1, 2, 3, 9, 10, 64, 65, 70):              # L > nt at the short traces
        f = rng.standard_normal(L)
        x = rng.standard_normal((2, nt))
        bound = rounding_bound(f, x)
        for o in origins(L):
            got = FR.apply(x, f, o)
            gott = FR.apply(x, f, o, transpose=True)
            for n in range(2):
                want = np.convolve(x[n], f)[o:o + nt]                        # (F x)[i] = conv(x, f)[i + o]
                wantt = np.convolve(x[n], f[::-1])[L - 1 - o:L - 1 - o + nt]   # (F^T x)[i] = conv(x, reversed f)[i + L - 1 - o]
                err = max(float(np.max(np.abs(got[n] - want))), float(np.max(np.abs(gott[n] - wantt))))
                worst = max(worst, err / bound)
                assert err <= bound, (L, o, err, bound)
    print(f"nt {nt}: largest distance from np.convolve {worst:.3f} of the bound")


@pytest.mark.parametrize("nt", (8, 9, 64, 65))
def test_transpose_is_the_transpose_in_every_bit(nt):
    rng = np.random.default_rng(nt)
    for L, os_ in ((5, (2,)), (nt + 3, origins(nt + 3))):
        f = rng.standard_normal(L)
        for o in os_:
            F, Ft = FR.matrix(nt, f, o), FR.matrix(nt, f, o, transpose=True)
            assert np.array_equal(Ft, F.T) and np.any(F != 0)
            # F[i][j] = f[i - j + o]: Toeplitz, entry for entry
            for i in range(nt):
                for j in range(nt):
                    k = i - j + o
                    assert F[i, j] == (f[k] if 0 <= k < L else 0.0)


@pytest.mark.parametrize("L, dt", [(64, 1.0), (64, 0.004), (257, 0.001), (2048, 0.004)])
def test_half_derivative_twice_is_the_first_difference(L, dt):
    g = rt_bench.half_derivative_taps(L, dt)
    got = np.convolve(g, g)[:L]
    want = np.zeros(L)
    want[0] = 1.0 / dt
    if L > 1:
        want[1] = -1.0 / dt
    err = float(np.max(np.abs(got - want)))
    print(f"L {L} dt {dt}: conv(g, g)[:L] - [1, -1, 0, ...] / dt = {err:.2e}, bound {L * 2.0 ** -52 / dt:.2e}")
    assert err <= L * 2.0 ** -52 / dt


@pytest.mark.parametrize("L, dt, hz", [(64, 0.004, 10.0), (64, 0.004, 31.0), (257, 0.001, 25.0), (9, 0.004, 60.0)])
def test_half_derivative_of_a_cosine(L, dt, hz):
    nt = L + 300
    w = 2.0 * np.pi * hz
    t = np.arange(nt) * dt
    x = np.cos(w * t)
    g = rt_bench.half_derivative_taps(L, dt)
    got = FR.apply(x, g, 0)
    want = (np.sqrt(1.0 - np.exp(-1j * w * dt)) / np.sqrt(dt) * np.exp(1j * w * t)).real
    tail = FR.half_derivative_tail(L, dt)
    err = float(np.max(np.abs(got[L:] - want[L:])))
    assert tail > 0
    print(f"L {L} dt {dt} {hz} Hz: |F cos - Re(G e^(i w t))| = {err:.3e} at i >= L, tail {tail:.3e}; sqrt(i w) differs from G by "
          f"{abs(np.sqrt(1j * w) - np.sqrt(1.0 - np.exp(-1j * w * dt)) / np.sqrt(dt)) / np.sqrt(w):.2e} of sqrt(w)")
    assert err <= tail + rounding_bound(g, x)


def test_tail_is_the_truncated_filters_dc_response():
    for L, dt in ((1, 1.0), (8, 0.004), (64, 0.004), (2048, 0.001)):
        g = rt_bench.half_derivative_taps(L, dt)
        assert g[0] > 0 and np.all(g[1:] < 0)
        tail = FR.half_derivative_tail(L, dt)
        assert abs(float(np.sum(g.astype(FR.LD))) - tail) <= L * U * float(np.sum(np.abs(g)))
        # sum over k < L of g_k = binomial(2 L - 2, L - 1) / 4^(L - 1) ~ 1 / sqrt(pi L): it falls slowly
        assert 0.5 / np.sqrt(np.pi * L * dt) < tail < 2.0 / np.sqrt(np.pi * L * dt)


# ---------------------------------------------------------------- rt_filter.h as a program of its own
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("filter_taps")
    src = os.path.join(ROOT, "tests", "native", "filter_taps.cpp")
    out = {}
    for name, flags in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall"] + flags + ["-o", exe, src])
        out[name] = exe
    return out


def hexes(v):
    return " ".join(float(a).hex() for a in v)


@pytest.mark.parametrize("build", ["plain", "san"])
def test_host_program_bit_for_bit(programs, build):
    """one run of the program per build: the half-derivative taps of three (L, dt), then F x and F^T x for nt = 1 .. 130 with
    filter lengths on both sides of nt and the three origins"""
    rng = np.random.default_rng(7)
    tap_cases = [(1, 1.0), (64, 0.004), (2048, 0.001)]
    cases = []
    for nt in range(1, 131):
        L = (1, 2, 5, 9, 64, 131, 140)[nt % 7]
        o = origins(L)[nt % len(origins(L))]
        cases.append((nt, L, o, rng.standard_normal(L), rng.standard_normal(nt)))
    text = f"{len(tap_cases)}\n" + "".join(f"{L} {float(dt).hex()}\n" for L, dt in tap_cases) + f"{len(cases)}\n"
    text += "".join(f"{nt} {L} {o}\n{hexes(f)}\n{hexes(x)}\n" for nt, L, o, f, x in cases)
    r = subprocess.run([programs[build]], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(tap_cases) + 2 * len(cases)

    def values(line, tag):
        w = line.split()
        assert w[0] == tag
        return np.array([float.fromhex(v) for v in w[1:]])
    for (L, dt), line in zip(tap_cases, lines):
        taps = values(line, "taps")
        lib_taps = rt_bench.half_derivative_taps(L, dt)
        assert taps.shape == lib_taps.shape and taps.tobytes() == lib_taps.tobytes()
    for i, (nt, L, o, f, x) in enumerate(cases):
        y, yt = values(lines[len(tap_cases) + 2 * i], "y"), values(lines[len(tap_cases) + 2 * i + 1], "yt")
        want, wantt = FR.apply(x, f, o), FR.apply(x, f, o, transpose=True)
        assert y.shape == want.shape and y.tobytes() == want.tobytes(), (nt, L, o)
        assert yt.shape == wantt.shape and yt.tobytes() == wantt.tobytes(), (nt, L, o)
