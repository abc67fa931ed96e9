"""GPU: the illumination map of a Kirchhoff handle (rtmi_kirchhoff_illumination, _dev; rt_bench.Kirchhoff.illumination /
illumination_device; include/rtmi.h) against the numpy restatement on the handle's own tables
(tests/lsqr_weighted_ref.illumination) bit for bit on every kind of handle -- one arrival, amplitudes and weights, 3 angle bins,
K = 2 with kmah, anti-aliased with 2 levels and holes in pt -- with the count of contributing pairs; on the handles where it is
diag(L^T L), against the squared norms of model_device's images of all 30 unit models; the device-pointer entry against the host
one, twice in a row, and tables that are all NaN."""
import ctypes as C

import numpy as np
import pytest

import kirchhoff_aa_ref as KA
import kirchhoff_multi_ref as KM
import lsqr_weighted_ref as WR
from lsqr_weighted_ref import DT, NT, tiny_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = C.c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


@pytest.fixture(scope="module")
def torch(rb):
    import torch
    assert torch.cuda.is_available()
    return torch


# kind -> (karr, kwargs of small_case, levels or None, the handle takes 3-D tables): 960 nodes, three full blocks and a partial one
KINDS = {
    "plain": (1, dict(holes=True), None, True),
    "amp_w": (1, dict(amp=True, w=True, holes=True), None, True),
    "bins3": (1, dict(nbin=3, amp=True, holes=True), None, True),
    "multi2_kmah": (2, dict(amp=True, kmah=True, holes=True), None, False),
    "aa2": (1, dict(amp=True, holes=True, pt_holes=True), KA.HW8[:2], False),
}


def make(rb, kind):
    karr, skw, hw, flat = KINDS[kind]
    pt = aa = None
    if hw is None:
        T, isrc, irec, kw = KM.small_case(karr, seed=5, **skw)
    else:
        T, pt, aa, isrc, irec, kw = KA.small_case(karr, hw=hw, seed=5, **skw)
    cut = (lambda a: None if a is None else a[:, 0]) if flat else (lambda a: a)
    op = rb.Kirchhoff(cut(T), isrc, irec, KM.SM_NT, KM.SM_DT, amp=cut(kw["amp"]), theta=cut(kw["theta"]), kmah=kw["kmah"],
                      weights=kw["w"], nbin=kw["nbin"], dopen=kw["dopen"], pt=pt, antialias=aa)
    return op, (T, isrc, irec, kw, pt)


@pytest.mark.parametrize("kind", list(KINDS))
def test_illumination_equals_the_restatement_bit_for_bit(rb, torch, kind):
    op, (T, isrc, irec, kw, pt) = make(rb, kind)
    want, count = WR.illumination(T, isrc, irec, KM.SM_NT, KM.SM_DT, pt=pt, **kw)
    got, st = op.illumination(stats=True)
    again = op.illumination()
    dev, sd = op.illumination_device(stats=True)
    print(f"{kind}: {st['contributing']} of {st['pairs']} pairs contribute, kernel {st['kernel_ms']:.3f} ms; {int((got == 0).sum())} of "
          f"{got.size} values dark, max {got.max():.6e}")
    assert got.shape == ((op.nb, op.ny, op.nx) if op.nbin else (op.ny, op.nx))
    assert got.tobytes() == want.reshape(got.shape).tobytes()
    assert st["contributing"] == count > 0 and st["pairs"] == op.N * op.ny * op.nx * max(op.karr, 1) ** 2
    assert again.tobytes() == got.tobytes()
    assert dev.is_cuda and dev.dtype == torch.float64 and dev.cpu().numpy().tobytes() == got.tobytes()
    assert sd["contributing"] == count
    assert np.all(got >= 0) and np.any(got > 0)
    # the operator pair is untouched by the call: migrate of ones counts the same pairs
    d = np.ones((op.N, op.nt))
    mig = op.migrate_channels(d, d if op.has_kmah else None, stats=True)[1] if op.karr else op.migrate(d, stats=True)[1]
    assert mig["contributing"] == count
    op.close()


@pytest.mark.parametrize("kind", ["plain", "amp"])
def test_illumination_is_the_squared_norm_of_every_column(rb, torch, kind):
    """P = 4, 6 x 5 nodes, N = 9, nt = 32: sum_k (L e_j)_k^2 from model_device for all 30 unit models"""
    T, isrc, irec, kw = tiny_case(amp=kind == "amp")
    op = rb.Kirchhoff(T, isrc, irec, NT, DT, amp=kw["amp"], weights=kw["w"])
    got = op.illumination()
    four = {k: (v[:, None] if k == "amp" and v is not None else v) for k, v in kw.items()}
    assert got.tobytes() == WR.illumination(T[:, None], isrc, irec, NT, DT, **four)[0].reshape(got.shape).tobytes()
    want = np.empty(got.size)
    for j in range(got.size):
        e = torch.zeros(got.size, dtype=torch.float64, device="cuda")
        e[j] = 1.0
        col = op.model_device(e.reshape(op.ny, op.nx))
        want[j] = float((col * col).sum().item())
    want = want.reshape(got.shape)
    lit = want > 0
    err = float(np.max(np.abs(got[lit] - want[lit]) / want[lit]))
    print(f"{kind}: {int(lit.sum())} of 30 columns lit, largest relative distance from sum model_device(e_j)^2 {err:.3e}")
    assert got.size == 30 and lit.any() and np.array_equal(got == 0.0, ~lit)
    assert err <= 1e-12
    op.close()


def test_tables_that_are_all_nan_give_plus_zero(rb):
    T, isrc, irec, kw = tiny_case()
    op = rb.Kirchhoff(np.full_like(T, np.nan), isrc, irec, NT, DT)
    got, st = op.illumination(stats=True)
    assert st["contributing"] == 0 and not got.any() and not np.signbit(got).any()
    op.close()


def test_illumination_scale_inside_the_solver(rb):
    """col_scale="illumination" is 1 / sqrt(illum + eps max(illum)) of the handle's map, dark values masked"""
    op, _ = make(rb, "plain")
    d = np.random.default_rng(9).standard_normal((op.N, op.nt))
    ill = op.illumination()
    scale = rb.illumination_scale(ill, 1e-2)
    assert np.array_equal(scale == 0.0, ill == 0.0)
    a = op.lsqr(d, 3, history=True, col_scale="illumination", eps=1e-2)
    b = op.lsqr(d, 3, history=True, col_scale=scale)
    assert a["x"].tobytes() == b["x"].tobytes() and np.array_equal(a["history"], b["history"])
    assert not a["x"][ill == 0.0].any()
    op.close()
