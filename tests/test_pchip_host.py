"""scipy's PCHIP as the device restates it (raytracing_amd/csrc/rt_pchip.h: k_isochrone, k_nodes and k_fine of wavefront.hip
all go through it) checked on the CPU: the header compiled for the host with g++ (tests/native/pchip_check.cpp) against the
np.longdouble restatement tests/pchip_ref.py on its RULE_SETS, which between them take every derivative rule.  The bound is
the device's own, pchip_ref.DEVICE_BOUND in eps x scale (scale: the largest |value| of the set; for derivatives the largest
|derivative| at the set's points).  No GPU involved."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pchip_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def pchiplib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pchip") / "libpchip_check.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "native", "pchip_check.cpp")])
    L = C.CDLL(so)
    L.pchip_derivs.argtypes = [C.c_long, _dp, _dp, _dp]
    L.pchip_eval.argtypes = [C.c_long, _dp, _dp, C.c_long, _dp, _dp, _dp, _dp]
    return L


def _ptr(a):
    return a.ctypes.data_as(_dp)


def _eps_scale(a, b, scale):
    """largest |a - b| in units of eps x scale"""
    worst = float(np.max(np.abs(np.asarray(a, dtype=P.LD) - np.asarray(b, dtype=P.LD))))
    return worst / (P.EPS * scale) if worst else 0.0


def test_header_against_the_restatement_on_every_rule(pchiplib):
    seen = collections.Counter()
    worst_d = worst_v = 0.0
    for t, v, rules in P.RULE_SETS:
        t, v = np.array(t), np.array(v)
        n = len(t)
        d, lab, near = P.derivatives(t, v)
        assert list(lab) == rules and not near.any()
        seen.update(rules)
        got_d = np.empty(n)
        pchiplib.pchip_derivs(n, _ptr(t), _ptr(v), _ptr(got_d))
        dscale = float(np.abs(d).max())
        e_d = _eps_scale(got_d, d, dscale)
        # every knot, every interval midpoint, 7 equally spaced abscissae
        q = np.concatenate([t, 0.5 * (t[1:] + t[:-1]), np.linspace(t[0], t[-1], 7)])
        powers, horner, slope = np.empty(len(q)), np.empty(len(q)), np.empty(len(q))
        pchiplib.pchip_eval(n, _ptr(t), _ptr(v), len(q), _ptr(q), _ptr(powers), _ptr(horner), _ptr(slope))
        want = P.evaluate(t, v, d, q)
        scale = float(np.abs(v).max())
        e_v = max(_eps_scale(powers, want, scale), _eps_scale(horner, want, scale))
        # k_nodes' rule: the derivative of the interpolant at the last breakpoint, from the last interval's right end
        e_s = _eps_scale(slope[n - 1:n], P.evaluate(t, v, d, t[-1:], nu=1), dscale)
        print(f"{'-'.join(rules)}: derivatives {e_d:.2f}, values {e_v:.2f}, slope at the last breakpoint {e_s:.2f} eps*scale")
        assert e_d <= P.DEVICE_BOUND and e_v <= P.DEVICE_BOUND and e_s <= P.DEVICE_BOUND
        worst_d, worst_v = max(worst_d, e_d, e_s), max(worst_v, e_v)
    print(f"worst: derivatives {worst_d:.2f}, values {worst_v:.2f} eps*scale; rules {dict(seen)}")
    assert all(seen[r] >= 1 for r in P.LABELS) and len(P.LABELS) == 7
