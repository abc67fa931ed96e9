"""CPU: the restatement of the anti-aliased Kirchhoff pair (tests/kirchhoff_aa_ref.py) against itself and against the closed forms
of v = 18 + 2 y: its degenerate cases are kirchhoff_multi_ref's bits; F_k is a symmetric matrix; the loop and the matrix are
transposes; a slope on a threshold selects that level; position_slope is the derivative of the traveltime in the position; and
the acceptance case of DESIGN.md 20 -- a zero-offset section of a flat reflector, migrated plainly and anti-aliased."""
import numpy as np
import pytest

import kirchhoff_aa_ref as KA
import kirchhoff_multi_ref as KM
import kirchhoff_ref as K1
from raytracing_amd import rt_bench


@pytest.mark.parametrize("degenerate", ["nlev 1", "lengths 0"])
@pytest.mark.parametrize("case", [(1, 0, False), (2, 5, True), (3, 0, True)])
def test_degenerate_cases_are_the_multi_restatement_bit_for_bit(degenerate, case):
    karr, nbin, kmah = case
    T, pt, aa, isrc, irec, kw = KA.small_case(karr, nbin=nbin, amp=True, w=True, kmah=kmah, holes=True, seed=3 + karr)
    aa = dict(aa, hw=(0,)) if degenerate == "nlev 1" else dict(hw=KA.HW8, asrc=0.0, arec=0.0, amid=0.0)
    rng = np.random.default_rng(1)
    d0, d1 = rng.standard_normal((2, len(isrc), KM.SM_NT))
    img, cnt = KA.migrate(T, pt, aa, isrc, irec, d0, d1 if kmah else None, KM.SM_DT, **kw)
    ref, cref = KM.migrate(T, isrc, irec, d0, d1 if kmah else None, KM.SM_DT, **kw)
    assert np.array_equal(img, ref) and cnt == cref
    L = KA.matrix(T, pt, aa, isrc, irec, KM.SM_NT, KM.SM_DT, **kw)
    Lref = KM.matrix(T, isrc, irec, KM.SM_NT, KM.SM_DT, **kw)
    assert (L != Lref).nnz == 0


@pytest.mark.parametrize("nt", [5, 64])
@pytest.mark.parametrize("k", [1, 3, 16])
def test_the_triangle_is_a_symmetric_matrix(k, nt):
    F = KA.tri_matrix(nt, k)
    assert np.array_equal(F, F.T)
    i, j = np.indices((nt, nt))
    assert np.array_equal(F, np.maximum(k + 1 - np.abs(i - j), 0) * (1.0 / ((k + 1.0) * (k + 1.0))))
    x = np.random.default_rng(k).standard_normal((3, nt))
    assert np.max(np.abs(KA.tri(x, k) - x @ F)) <= 1e-15 * (2 * k + 1) * np.max(np.abs(x))
    assert np.array_equal(KA.tri(x, 0), x)


@pytest.mark.parametrize("case", [(1, 0, False, False), (1, 5, True, True), (3, 0, True, False), (3, 5, True, True)])
def test_the_loop_and_the_matrix_are_transposes(case):
    karr, nbin, kmah, pt_holes = case
    T, pt, aa, isrc, irec, kw = KA.small_case(karr, pt_holes=pt_holes, nbin=nbin, amp=True, w=True, kmah=kmah, holes=True, seed=11 + karr)
    seen, beyond = KA.levels_hit(T, pt, aa, isrc, irec, KM.SM_NT, kw)
    assert seen == set(range(len(KA.HW8))) and beyond
    N, nt = len(isrc), KM.SM_NT
    rng = np.random.default_rng(4)
    d0, d1 = rng.standard_normal((2, N, nt))
    if not kmah:
        d1 = np.zeros_like(d1)
    m = rng.standard_normal((max(nbin, 1),) + T.shape[2:])
    L = KA.matrix(T, pt, aa, isrc, irec, nt, KM.SM_DT, **kw)
    img, cnt = KA.migrate(T, pt, aa, isrc, irec, d0, d1 if kmah else None, KM.SM_DT, **kw)
    d = np.concatenate([d0.reshape(-1), d1.reshape(-1)])
    lhs, rhs = float((L @ m.reshape(-1)) @ d), float(m.reshape(-1) @ img.reshape(-1))
    scale = float(np.abs(d) @ (abs(L) @ np.abs(m.reshape(-1))))
    full = KM.migrate(T, isrc, irec, d0, d1 if kmah else None, KM.SM_DT, **kw)[1]
    print(f"{case}: contributing {cnt} (of {full} with every pt finite), |diff| / sum|terms| {abs(lhs - rhs) / scale:.2e}")
    assert (cnt < full) == pt_holes
    assert abs(lhs - rhs) <= 1e-13 * scale
    assert np.max(np.abs(L.T @ d - img.reshape(-1))) <= 1e-13 * np.max(abs(L).T @ np.abs(d))


def test_a_slope_on_a_threshold_selects_that_level():
    dt, arec = 2.0 ** -10, 0.5
    hw = KA.HW8
    pr = np.array([float(h) for h in hw]) * dt / arec            # exact: powers of two throughout
    assert np.array_equal(KA.level(np.zeros(8), pr, hw, dt, arec=arec), np.arange(8))
    assert np.array_equal(KA.level(np.zeros(8), -pr, hw, dt, arec=arec), np.arange(8))
    up = np.nextafter(pr, np.inf)
    up[0] = 1e-300                                               # the next double after 0 is lost in the product with arec
    assert np.array_equal(KA.level(np.zeros(8), up, hw, dt, arec=arec), np.minimum(np.arange(8) + 1, 7))
    assert KA.level(0.0, 1e9, hw, dt, arec=arec) == 7 and KA.level(0.0, np.inf, hw, dt, arec=arec) == 7
    # the three terms: the source's, the receiver's, the midpoint's sum
    assert KA.level(4 * dt, 0.0, hw, dt, asrc=1.0) == 3 and KA.level(4 * dt, 0.0, hw, dt, arec=1.0) == 0
    assert KA.level(4 * dt, -4 * dt, hw, dt, amid=1.0) == 0 and KA.level(4 * dt, 4 * dt, hw, dt, amid=1.0) == 4
    assert KA.level(4 * dt, 1 * dt, hw, dt, asrc=1.0, arec=16.0, amid=1.0) == 5
    assert KA.level(5.0, 5.0, (0,), dt, 1.0, 1.0, 1.0) == 0


def test_position_slope_is_the_derivative_in_the_position():
    th0 = KA.closed_theta0()
    pt = rt_bench.position_slope({"theta0": th0}, np.full(len(K1.POS_X), KA.closed_n()))
    ref = KA.closed_pt_central()
    e = np.max(np.abs(pt - ref)) / np.max(np.abs(pt))
    print(f"position_slope against the central difference of vert_T (h = 1e-6): {e:.2e} of max|pt| = {np.max(np.abs(pt)):.4f}")
    assert pt.shape == K1.closed_T().shape and e <= 1e-7
    # a 4-D table and another direction
    p4 = rt_bench.position_slope({"theta0": np.stack([th0, th0], axis=1)}, np.full(len(K1.POS_X), KA.closed_n()), direction=(0.0, 1.0))
    assert p4.shape == (48, 2) + th0.shape[1:] and np.array_equal(p4[:, 0], -KA.closed_n() * np.sin(th0))
    with pytest.raises(ValueError, match="one value per position"):
        rt_bench.position_slope({"theta0": th0}, np.ones(3))


def test_acceptance_flat_reflector_zero_offset():
    """Artefact / reflector of the plain migration 0.1778; anti-aliased over plain 0.028 in the prototype, reflector kept 0.963."""
    isrc, irec, d, amid = KA.acceptance_data()
    T = K1.closed_T()
    pt = rt_bench.position_slope({"theta0": KA.closed_theta0()}, np.full(len(K1.POS_X), KA.closed_n()))
    plain, _ = K1.migrate(T, isrc, irec, d, K1.DT)
    aa, _ = KA.migrate(T[:, None], pt[:, None], dict(hw=KA.ACC_HW, asrc=0.0, arec=0.0, amid=amid), isrc, irec, d, None, K1.DT)
    rp, ap = KA.acceptance_figures(plain)
    ra, aa_ = KA.acceptance_figures(aa)
    print(f"plain: artefact / reflector {ap / rp:.4f}; anti-aliased: {aa_ / ra:.4f}; ratio {(aa_ / ra) / (ap / rp):.4f}; "
          f"reflector kept {ra / rp:.4f}")
    assert (aa_ / ra) / (ap / rp) <= 0.1
    assert ra / rp >= 0.9
