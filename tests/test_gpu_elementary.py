"""GPU: the device's restatements of numpy's float64 arctan2 (rt::ex::atan2_, rt_exact.h, with its VRCP14PD table as k_rcp14_init
decodes it) and of numpy's array exp (np_exp, field.hip) against the oracle's, on uint64 views, on the argument sets of
tests/elementary_sets.py -- on which tests/test_elementary_sets.py holds the oracle to numpy itself.  Where this host's numpy
dispatches to SVML the device is compared with np.arctan2 and np.exp directly as well."""
import os
import subprocess
import sys

import numpy as np
import pytest

import elementary_sets as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench
    return rt_bench


@pytest.fixture(scope="module")
def O():
    from oracle import rt_oracle
    return rt_oracle


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _one_exact_step(rb):
    """A batch of a method that steps with atan2_ (op4): rtmi_batch_create decodes the table on the batch's stream"""
    F = rb.Field.build("vert_heterogeneous", (-1, 1, -2, 0), 0.07)
    b = rb.Batch(F, 4, rb.DELTA_S, 16, (-1, 1, -2, 0), 1, np.linspace(0.1, 1.4, 64), -0.5, -1.0, record_stride=0)
    b.step(1)
    fin = b.final()
    b.close(); F.close()
    return fin


def test_device_table_is_the_headers(rb):
    """All 65 536 entries of g_rcp14 as this process's device holds them, once a batch exists (whoever decoded it first) ..."""
    T = E.rcp14_table()
    _one_exact_step(rb)
    assert np.array_equal(rb.device_rcp14_table(), T)
    assert np.array_equal(rb.device_rcp14_table(), T)


_CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import elementary_sets as E
from raytracing_amd import rt_bench as rb
import test_gpu_elementary as G
T = E.rcp14_table()
first = rb.device_rcp14_table()              # nothing on this process's device has asked for the table yet
fin = G._one_exact_step(rb)
after = rb.device_rcp14_table()
print("table", int(np.sum(first != T)), int(np.sum(after != T)), bool(np.isfinite(fin[:3]).all()))
"""


def test_device_table_when_the_diagnostic_decodes_it_first():
    """... and in a fresh process, where rtmi_debug_rcp14_table itself is the table's first user (null stream) and a batch comes
    after it: the same 65 536 entries before and after."""
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=E.ROOT, tests=tests)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "table 0 0 True" in r.stdout, r.stdout


def test_arctan2_main_path_is_the_oracles_bits(rb, O):
    """Both operands in [2^-1020, 2^993): every table entry under both signs of x, five base points x four quadrants, the four
    octant switches at equality and +-1 ulp, 600 decades, the hand-over's inner side."""
    y, x = E.arctan2_pairs()
    main = E.arctan2_main(y, x)
    y, x = y[main], x[main]
    assert E.rcp14_indices_read(y, x).size == 65536
    d = rb.device_arctan2(y, x)
    bad = _bits(d) != _bits(O.np_arctan2(y, x))
    print(f"arctan2 main path: {bad.sum()} of {y.size} pairs differ from the oracle")
    assert not bad.any(), f"{bad.sum()} of {y.size} differ; first (y, x) = {y[bad][:3]}, {x[bad][:3]}"
    if E.avx512_skx():
        bad = _bits(d) != _bits(np.arctan2(y, x))
        assert not bad.any(), f"{bad.sum()} of {y.size} differ from np.arctan2"


def test_arctan2_outside_the_main_path(rb, O):
    """SVML's scalar fall-back (libm's atan2 in the oracle, ocml's on the device): zeros and infinities give the exactly
    representable multiples of pi/4 with y's sign, bit for bit; NaN in, NaN out; everything else within 2 ulp -- the project's
    bound for ocml's atan2 against numpy's (tests/crossing_ref.py)."""
    y, x = E.arctan2_pairs()
    out = ~E.arctan2_main(y, x)
    gy, gx = E.arctan2_special_grid()
    y, x = np.concatenate([gy, y[out]]), np.concatenate([gx, x[out]])
    d, o = rb.device_arctan2(y, x), O.np_arctan2(y, x)
    nan = np.isnan(y) | np.isnan(x)
    assert nan.sum() == 19 and np.all(np.isnan(d[nan])) and np.all(np.isnan(o[nan]))
    exact = ~nan & ((y == 0) | (x == 0) | np.isinf(y) | np.isinf(x))
    assert exact.sum() == 56                    # 9 x 9 without NaN, less the 5 x 5 of finite non-zero operands
    assert np.array_equal(_bits(d[exact]), _bits(o[exact])), (y[exact][_bits(d[exact]) != _bits(o[exact])], x[exact][_bits(d[exact]) != _bits(o[exact])])
    rest = ~nan & ~exact
    u = E.ulp_distance(d[rest], o[rest])
    print(f"arctan2 fall-back: {np.sum(d[rest] != o[rest])} of {rest.sum()} finite pairs differ from the oracle, at most {u.max():.3g} ulp")
    assert rest.sum() > 8_000 and np.all(np.signbit(d[rest]) == np.signbit(o[rest]))
    assert u.max() <= 2, (u.max(), y[rest][np.argmax(u)], x[rest][np.argmax(u)])
    if E.avx512_skx():
        with np.errstate(invalid="ignore"):
            ref = np.arctan2(y, x)
        assert np.array_equal(_bits(d[exact]), _bits(ref[exact])) and E.ulp_distance(d[rest], ref[rest]).max() <= 2


def test_exp_main_path_is_the_oracles_bits(rb, O):
    """|x| < 0x1.61da04cbafe44p+9: dense, the 1/16 grid, the multiples of ln2/16 with both neighbours (the floor correction), the
    interface scenario's own arguments."""
    x = E.exp_main_args()
    d = rb.device_exp(x)
    bad = _bits(d) != _bits(O.np_exp(x))
    print(f"exp main path: {bad.sum()} of {x.size} arguments differ from the oracle")
    assert not bad.any(), f"{bad.sum()} of {x.size} differ; first x = {[v.hex() for v in x[bad][:4]]}"
    if E.avx512_skx():
        bad = _bits(d) != _bits(np.exp(x))
        assert not bad.any(), f"{bad.sum()} of {x.size} differ from np.exp"


def test_exp_outside_the_main_path_gives_the_same_field(rb, O):
    """|x| >= 707.7 (SVML's scalar fall-back: libm's exp in the oracle, ocml's on the device): last bits are not compared; the
    interface scenario's n from either e is the same bits, and e is inf, 0 or NaN in the same places."""
    x = E.exp_outside_args()
    d, o = rb.device_exp(x), O.np_exp(x)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(_bits(E.interface_n(d)), _bits(E.interface_n(o)))
    for f in (np.isinf, np.isnan, lambda v: v == 0):
        assert np.array_equal(f(d), f(o))
    assert np.isinf(d).sum() > 1000 and (d == 0).sum() > 1000 and np.isnan(d).sum() == 1
