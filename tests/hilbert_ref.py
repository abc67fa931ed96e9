"""Restatement of the device's Hilbert transform (include/rtmi.h; raytracing_amd/csrc/rt_hilbert.h): the taps
by the formula in np.longdouble, and y = H x as a plain ascending loop over the taps with every subtract, product and add a separate
fp64 operation (numpy forms each as a temporary of its own).  The loop takes the taps as an argument: y is defined bit for bit given
the taps, and the taps are held to the formula separately.  Test infrastructure."""
import numpy as np

LD = np.longdouble
PI = LD(4) * np.arctan(LD(1))


def ntaps(n):
    return max((int(n) - 1) // 2, 0)


def taps_formula(n):
    """c_1 .. c_K in np.longdouble (not rounded to fp64).  n even: (2 / n) cot(a_k) at odd k, exactly 0 at even k; n odd:
    (cot(a_k) - (-1)^k / sin(a_k)) / n, written by the half angle -- cot(a) + 1 / sin(a) = cot(a / 2) at odd k and
    cot(a) - 1 / sin(a) = -tan(a / 2) at even k, the same numbers without the cancellation of cos(a) - 1 at small a."""
    n = int(n)
    k = np.arange(1, ntaps(n) + 1)
    a = PI * k.astype(LD) / LD(n)
    odd_k = (k & 1) == 1
    if n % 2 == 0:
        return np.where(odd_k, LD(2) * np.cos(a) / (LD(n) * np.sin(a)), LD(0))
    return np.where(odd_k, np.cos(a / 2) / (LD(n) * np.sin(a / 2)), -np.tan(a / 2) / LD(n))


def taps_literal(n):
    """the formula as include/rtmi.h writes it, in np.longdouble: at an odd n it cancels at small a_k"""
    n = int(n)
    k = np.arange(1, ntaps(n) + 1)
    a = PI * k.astype(LD) / LD(n)
    if n % 2 == 0:
        return np.where((k & 1) == 1, LD(2) / LD(n) * np.cos(a) / np.sin(a), LD(0))
    sign = np.where((k & 1) == 1, LD(-1), LD(1))
    return (np.cos(a) / np.sin(a) - sign / np.sin(a)) / LD(n)


def hilbert(x, taps):
    """y = H x along the last axis: from +0.0, k ascending, the taps that are 0 skipped"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    taps = np.asarray(taps, dtype=np.float64)
    assert taps.shape == (ntaps(n),)
    y = np.zeros(x.shape)
    for k in range(1, taps.size + 1):
        c = float(taps[k - 1])
        if c == 0.0:
            continue
        d = np.roll(x, k, axis=-1) - np.roll(x, -k, axis=-1)      # x[(i - k) mod n] - x[(i + k) mod n]
        p = c * d
        y = y + p
    return y


def apply(x, taps, add=None, negate=False):
    """the kernel's result: (add or +0) +- y, with add one more fp64 add, without it y or its exact negation"""
    y = hilbert(x, taps)
    if negate:
        y = -y
    return y if add is None else np.asarray(add, dtype=np.float64) + y


def matrix(n, taps):
    """H as a matrix, column j = H e_j"""
    return hilbert(np.eye(n), taps).T
