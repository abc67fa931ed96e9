"""CPU: the restatement of rtmi_kirchhoff_lsqr (tests/kirchhoff_lsqr_ref.py).  fix_norm against an exact
norm, under permutations and at the ends of its range; lsqr_loop against scipy's lsqr on the small Kirchhoff matrix; the scalar
recurrence of raytracing_amd/csrc/rt_lsqr.h, built as a program of its own (plain, and with the address and undefined-behaviour
sanitizers), against the restatement's scalars bit for bit."""
import math
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import kirchhoff_lsqr_ref as R
import kirchhoff_multi_ref as KM
import kirchhoff_ref as K1
from conftest import ROOT


def bits(v):
    return struct.pack("<d", float(v))


def exact_norm(x):
    """sqrt of the exact sum of exact squares, by way of an integer square root with 700 fractional bits (far below half an ulp)"""
    s = sum(Fraction(float(v)) ** 2 for v in x)
    if s == 0:
        return 0.0
    shift = 2 * 700
    n = (s.numerator << shift) // s.denominator
    return float(Fraction(math.isqrt(n), 1 << (shift // 2)))


@pytest.mark.parametrize("n", [1, 255, 257, 65537])
def test_fix_norm_against_the_exact_norm(n):
    """relative error <= n 2^-58 + 2^-52: the quantum is at most M^2 2^-56, so half a quantum per term is at most M^2 2^-57 against
    a sum of at least M^2, n 2^-57 of the sum in all and half of that after the square root; one rounding per product (2^-53 of
    the sum, 2^-54 of the norm), one of the sum and one of the square root are the rest"""
    rng = np.random.default_rng(n)
    worst = 0.0
    for x in (rng.standard_normal(n), rng.standard_normal(n) * 2.0 ** rng.integers(-30, 1, n), np.full(n, 0.7391)):
        got, want = R.fix_norm(x), exact_norm(x)
        err = abs(got - want) / want
        worst = max(worst, err)
        assert err <= n * 2.0 ** -58 + 2.0 ** -52, (n, err)
        assert bits(R.fix_norm(rng.permutation(x))) == bits(got)
        assert bits(R.fix_norm(-x)) == bits(got)
    print(f"n {n}: largest relative error of fix_norm {worst:.3e} (bound {n * 2.0 ** -58 + 2.0 ** -52:.3e})")


def test_fix_norm_zero_and_range():
    assert bits(R.fix_norm(np.zeros(7))) == bits(0.0)
    assert R.fix_norm(np.zeros(7), with_exponent=True) == (0.0, 0)
    for M in (1e200, 1e-200):
        with pytest.raises(R.NormRange):
            R.fix_norm(np.array([0.5 * M, -M, 0.0]))
    # the ends of the range that still work
    assert R.fix_norm(np.array([1e150, 1e150])) == pytest.approx(math.sqrt(2) * 1e150, rel=1e-15)
    assert R.fix_norm(np.array([1e-150, 1e-150])) == pytest.approx(math.sqrt(2) * 1e-150, rel=1e-15)
    # in the solver the case is an istop of its own
    A = np.array([[1e200, 0.0], [0.0, 1.0]])
    out = R.lsqr_loop(lambda v: A @ v, lambda u: A.T @ u, np.array([1.0, 1.0]), 3)
    assert out["istop"] == R.LSQR_RANGE == 8


@pytest.fixture(scope="module")
def small():
    T, isrc, irec, kw = KM.small_case(1)
    L = K1.matrix(T[:, 0], isrc, irec, KM.SM_NT, KM.SM_DT)
    m = np.random.default_rng(21).standard_normal(L.shape[1])
    return L, L @ m


def run(L, d, iter_lim, scalars=None, **kw):
    return R.lsqr_loop(lambda v: L @ v, lambda u: L.T @ u, d, iter_lim, scalars=scalars, **kw)


@pytest.mark.parametrize("damp", [0.0, 0.1])
def test_lsqr_loop_against_scipy(small, damp):
    from scipy.sparse.linalg import lsqr
    L, d = small
    assert L.shape == (23 * 64, 960)
    got = run(L, d, 10, damp=damp)
    ref = lsqr(L, d, damp=damp, atol=0, btol=0, conlim=0, iter_lim=10)
    rg = float(np.linalg.norm(L @ got["x"] - d) / np.linalg.norm(d))
    rr = float(np.linalg.norm(L @ ref[0] - d) / np.linalg.norm(d))
    ex = float(np.max(np.abs(got["x"] - ref[0])) / np.max(np.abs(ref[0])))
    print(f"damp {damp}: residual ratio of the restatement {rg:.10f}, of scipy {rr:.10f}; largest relative difference of x {ex:.3e}; "
          f"r1norm {got['r1norm']:.12e} against {ref[3]:.12e}, anorm {got['anorm']:.12e} against {ref[5]:.12e}")
    assert got["itn"] == ref[2] == 10 and got["istop"] == ref[1] == 7
    assert abs(rg - rr) <= 1e-6 * rr
    assert got["history"].shape == (10, 4)
    for mine, theirs in ((got["r1norm"], ref[3]), (got["r2norm"], ref[4]), (got["anorm"], ref[5]), (got["arnorm"], ref[7])):
        assert abs(mine - theirs) <= 1e-9 * abs(theirs)


def test_lsqr_loop_stops_where_scipy_does(small):
    from scipy.sparse.linalg import lsqr
    L, d = small
    got = run(L, d, 500, atol=1e-3, btol=1e-3)
    ref = lsqr(L, d, atol=1e-3, btol=1e-3, conlim=0, iter_lim=500)
    print(f"atol = btol = 1e-3: itn {got['itn']} istop {got['istop']}; scipy itn {ref[2]} istop {ref[1]}")
    assert (got["itn"], got["istop"]) == (ref[2], ref[1])
    assert got["istop"] in (1, 2) and got["itn"] < 500


def test_lsqr_loop_zero_data(small):
    from scipy.sparse.linalg import lsqr
    L, d = small
    got = run(L, np.zeros_like(d), 10)
    ref = lsqr(L, np.zeros_like(d), iter_lim=10)
    assert got["itn"] == ref[2] == 0 and got["istop"] == ref[1] == 0
    assert got["x"].shape == ref[0].shape and not got["x"].any() and not ref[0].any()
    assert got["history"].shape == (0, 4)
    # data the operator's transpose annihilates: the other early return
    Z = L * 0.0
    got = R.lsqr_loop(lambda v: Z @ v, lambda u: Z.T @ u, d, 10)
    assert got["itn"] == 0 and got["istop"] == 0 and not got["x"].any()


def test_a_norm_out_of_range_inside_the_loop_abandons_its_iteration(small):
    """the 7th and the 8th norm are the u and the v of the third iteration: two iterations stand either way, with the scalars and
    the x a run of two iterations ends with (but for istop and the iteration limit's own test)"""
    L, d = small
    two = run(L, d, 3)                           # a limit of 3: the second iteration does not stop the run
    for fail_at in (7, 8):
        calls = []

        def norm(x):
            calls.append(1)
            if len(calls) == fail_at:
                raise R.NormRange("made up")
            return R.fix_norm(x)

        got = R.lsqr_loop(lambda v: L @ v, lambda u: L.T @ u, d, 10, norm=norm)
        assert got["istop"] == R.LSQR_RANGE and got["itn"] == 2 and got["history"].shape == (2, 4)
        assert np.array_equal(got["history"], two["history"][:2])
        ref = run(L, d, 2)
        assert np.array_equal(got["x"], ref["x"])
        for key in ("r1norm", "r2norm", "anorm", "arnorm"):
            assert bits(got[key]) == bits(ref[key]), key


def test_fix_norm_when_the_sum_of_squares_exceeds_the_range():
    """max|x|^2 is in range, the sum of the squares is not: the norm is still finite, the root taken with the even part of the
    exponent outside"""
    x = np.full(1000, 1.2e154)
    got = R.fix_norm(x)
    want = math.sqrt(1000.0) * 1.2e154
    assert math.isfinite(got) and abs(got - want) <= 1e-15 * want
    x = np.full(1000, 1.6e-154)
    assert abs(R.fix_norm(x) - math.sqrt(1000.0) * 1.6e-154) <= 1e-15 * math.sqrt(1000.0) * 1.6e-154
    # and where both forms work they agree in every bit
    rng = np.random.default_rng(5)
    for k in range(20):
        y = rng.standard_normal(50) * 2.0 ** k
        nrm, e = R.fix_norm(y, with_exponent=True)
        S = sum(round(math.ldexp(p, -e)) for p in (y * y).tolist())
        assert bits(nrm) == bits(math.sqrt(math.ldexp(float(S), e)))


# ---------------------------------------------------------------- rt_lsqr.h as a program of its own
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("lsqr_scalars")
    src = os.path.join(ROOT, "tests", "native", "lsqr_scalars.cpp")
    out = {}
    for name, flags in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall"] + flags + ["-o", exe, src])
        out[name] = exe
    return out


@pytest.mark.parametrize("build", ["plain", "san"])
@pytest.mark.parametrize("case", [dict(damp=0.0), dict(damp=0.1), dict(damp=0.0, atol=1e-3, btol=1e-3, iter_lim=500)])
def test_scalar_recurrence_bit_for_bit(small, programs, build, case):
    L, d = small
    kw = dict(damp=0.0, atol=0.0, btol=0.0, iter_lim=10)
    kw.update(case)
    iter_lim = kw.pop("iter_lim")
    norms = []

    def norm(x):
        norms.append(R.fix_norm(x))
        return norms[-1]

    rec = []
    got = R.lsqr_loop(lambda v: L @ v, lambda u: L.T @ u, d, iter_lim, norm=norm, scalars=rec, **kw)
    assert len(norms) == 2 + 2 * got["itn"]
    text = " ".join([float(kw["damp"]).hex(), float(kw["atol"]).hex(), float(kw["btol"]).hex(), str(iter_lim)] + [v.hex() for v in norms])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")      # the leak checker needs ptrace
    p = subprocess.run([programs[build]], input=text, capture_output=True, text=True, env=env)
    assert p.returncode == 0 and p.stderr == "", p.stderr
    lines = p.stdout.strip().split("\n")
    assert lines[-1] == f"end {got['itn']} {got['istop']}"
    assert len(lines) - 1 == len(rec) == got["itn"]
    for line, want in zip(lines, rec):
        have = [float.fromhex(t) for t in line.split()]
        assert [bits(v) for v in have] == [bits(v) for v in want], (have, want)
