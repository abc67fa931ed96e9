"""CPU: the definition of the device's Hilbert transform (include/rtmi.h).  The library's taps
(rtmi_hilbert_taps, host only) against the formula in np.longdouble; the restatement tests/hilbert_ref.py against rt_bench.hilbert,
the FFT form of the same matrix; H[cos] = sin; the matrix's transpose is -H in every bit; rt_hilbert.h as a program of its own,
plain and under -fsanitize=address,undefined, against the library's taps and the restatement bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raytracing_amd import rt_bench

import hilbert_ref as HR

SIZES = (1, 2, 3, 4, 5, 8, 9, 64, 65, 250, 257, 1024, 9000, 16384)


@pytest.mark.parametrize("n", SIZES)
def test_taps_are_the_formula_rounded_once(n):
    taps = rt_bench.hilbert_taps(n)
    want = HR.taps_formula(n)
    assert taps.dtype == np.float64 and taps.shape == (HR.ntaps(n),) == want.shape
    if n % 2 == 0:
        assert not taps[1::2].any() and not np.signbit(taps[1::2]).any()      # exact +0.0 at the even k of an even n
        taps, want = taps[0::2], want[0::2]
    if taps.size == 0:
        return
    assert np.all(taps != 0.0) and np.all(np.isfinite(taps))
    ulp = np.spacing(np.abs(taps))
    err = float(np.max(np.abs(taps.astype(HR.LD) - want) / ulp.astype(HR.LD)))
    print(f"n {n}: {taps.size} taps that are not zero, largest distance from the formula {err:.3f} ulp")
    assert err <= 1.0


@pytest.mark.parametrize("n", SIZES)
def test_half_angle_form_is_the_formula_as_written(n):
    """taps_formula writes an odd n's taps by the half angle.  Against the formula as rtmi.h writes it, in np.longdouble: the
    literal form computes cos(a) -+ 1 with an absolute error of about 2^-64, which its division by sin(a) ~ a and by n leaves as
    2^-64 / (n a) absolute; 8 of those is the bound."""
    a, b = HR.taps_formula(n), HR.taps_literal(n)
    if a.size == 0:
        return
    k = np.arange(1, a.size + 1).astype(HR.LD)
    bound = 8 * HR.LD(2) ** -64 / (HR.PI * k) + 8 * HR.LD(2) ** -64 * np.abs(a)
    assert np.all(np.abs(a - b) <= bound)


@pytest.mark.parametrize("n", (2, 3, 4, 5, 8, 9, 64, 65, 250, 257, 1024))
def test_restatement_equals_the_fft_form(n):
    x = np.random.default_rng(100 + n).standard_normal((3, n))
    got = HR.hilbert(x, rt_bench.hilbert_taps(n))
    want = rt_bench.hilbert(x)
    scale = float(np.max(np.abs(want))) or 1.0
    err = float(np.max(np.abs(got - want))) / scale
    print(f"n {n}: time-domain form against the FFT form {err:.2e} of max|Hx|")
    assert err <= 1e-12
    if n <= 2:
        assert not got.any() and not np.signbit(got).any()


def test_cosine_becomes_sine():
    n = 256
    t = np.arange(n) / n
    got = HR.hilbert(np.cos(2 * np.pi * 5 * t), rt_bench.hilbert_taps(n))
    err = float(np.max(np.abs(got - np.sin(2 * np.pi * 5 * t))))
    print(f"H[cos 2 pi 5 t] - sin 2 pi 5 t at n = 256: {err:.2e}")
    assert err <= 1e-13


@pytest.mark.parametrize("n", (8, 9, 64, 65))
def test_transpose_is_minus_h_in_every_bit(n):
    H = HR.matrix(n, rt_bench.hilbert_taps(n))
    assert np.array_equal(H.T, -H)
    assert np.any(H != 0) and not np.diag(H).any()


def test_apply_adds_once_and_negates_exactly():
    n = 65
    rng = np.random.default_rng(5)
    x, add = rng.standard_normal((2, n)), rng.standard_normal((2, n))
    taps = rt_bench.hilbert_taps(n)
    y = HR.hilbert(x, taps)
    assert np.array_equal(HR.apply(x, taps), y) and np.array_equal(HR.apply(x, taps, negate=True), -y)
    assert np.array_equal(HR.apply(x, taps, add=add), add + y) and np.array_equal(HR.apply(x, taps, add=add, negate=True), add - y)


# ---------------------------------------------------------------- rt_hilbert.h as a program of its own
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("hilbert_taps")
    src = os.path.join(ROOT, "tests", "native", "hilbert_taps.cpp")
    out = {}
    for name, flags in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall"] + flags + ["-o", exe, src])
        out[name] = exe
    return out


@pytest.mark.parametrize("build", ["plain", "san"])
@pytest.mark.parametrize("n", (1, 2, 3, 4, 9, 64, 65, 250, 257))
def test_host_program_bit_for_bit(programs, build, n):
    x = np.random.default_rng(n).standard_normal(n)
    text = f"{n}\n" + " ".join(float(v).hex() for v in x) + "\n"
    r = subprocess.run([programs[build]], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].split()[0] == "taps" and lines[1].split()[0] == "y"
    taps = np.array([float.fromhex(v) for v in lines[0].split()[1:]])
    y = np.array([float.fromhex(v) for v in lines[1].split()[1:]])
    lib_taps = rt_bench.hilbert_taps(n)
    assert taps.shape == lib_taps.shape and taps.tobytes() == lib_taps.tobytes()
    want = HR.hilbert(x, lib_taps)
    assert y.shape == want.shape and y.tobytes() == want.tobytes()
