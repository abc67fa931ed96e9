"""Restatement of the device's trace filter (include/rtmi.h; raytracing_amd/csrc/rt_filter.h): y = F x and
y = F^T x as a plain ascending loop over the taps with every product and add a separate fp64 operation (numpy forms each as a
temporary of its own), terms outside the trace left out; and the half-derivative taps by their recurrence in np.longdouble.  Test
infrastructure."""
import numpy as np

LD = np.longdouble


def half_derivative_formula(L, dt):
    """g_k / sqrt(dt), k = 0 .. L - 1, in np.longdouble (not rounded to fp64): g_0 = 1, g_k = g_(k-1) (2 k - 3) / (2 k)"""
    g = np.empty(int(L), dtype=LD)
    s = LD(1) / np.sqrt(LD(dt))
    v = LD(1)
    for k in range(int(L)):
        if k > 0:
            v = v * LD(2 * k - 3) / LD(2 * k)
        g[k] = v * s
    return g


def half_derivative_tail(L, dt):
    """the absolute sum of the taps that L taps leave out, sum over k < L of g_k / sqrt(dt): the series sums to zero and every
    g_k with k >= 1 is negative"""
    return float(np.sum(half_derivative_formula(L, dt)))


def apply(x, taps, origin=0, transpose=False):
    """F x, or F^T x with transpose, along the last axis: from +0.0, k ascending, a term whose sample lies outside the trace
    left out"""
    x = np.asarray(x, dtype=np.float64)
    f = np.asarray(taps, dtype=np.float64)
    nt, o = x.shape[-1], int(origin)
    assert f.ndim == 1 and 0 <= o < f.size
    y = np.zeros(x.shape)
    for k in range(f.size):
        s = o - k if not transpose else k - o           # output i reads x[i + s]
        lo, hi = max(0, -s), min(nt, nt - s)            # the outputs whose sample is inside the trace
        if lo >= hi:
            continue
        p = float(f[k]) * x[..., lo + s:hi + s]
        y[..., lo:hi] = y[..., lo:hi] + p
    return y


def matrix(nt, taps, origin=0, transpose=False):
    """F (or F^T) as a matrix, column j = F e_j"""
    return apply(np.eye(nt), taps, origin, transpose).T
