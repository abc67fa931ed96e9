"""CPU: the numpy restatement of the Kirchhoff pair (tests/kirchhoff_ref.py) on closed-form tables.  The standard case images
its scatterer where it is, with the amplitude linear interpolation of a 60 Hz wavelet at 1 ms leaves, and splits it over the
opening-angle bins as the closed-form angles say; the pair is adjoint to rounding, NaN holes included.  Measured values:
DESIGN.md section 14."""
import numpy as np
import pytest

import kirchhoff_ref as K


@pytest.fixture(scope="module")
def std():
    isrc, irec = K.geometry()
    return {"T": K.closed_T(), "theta": K.closed_theta(), "isrc": isrc, "irec": irec, "data": K.scatterer_data(isrc, irec)}


def test_closed_form_direction_is_the_direction_of_grad_T(std):
    """atan2(-sigma (x - xc), sigma (y + 9)) against the direction of the finite-difference gradient of the closed-form T, away
    from the grid's rim"""
    T, th = std["T"][10], std["theta"][10]
    gy, gx = np.gradient(T, 0.025, 0.025)
    d = np.arctan2(gy, gx) - th
    d = np.abs(d - K.TWO_PI * np.rint(d / K.TWO_PI))[2:-2, 2:-2]
    print(f"direction against grad T: {d.max():.2e}")
    assert d.max() <= 1e-3


def test_standard_case_images_the_scatterer(std):
    N = len(std["isrc"])
    assert N == 576 and std["T"].shape == (48, 101, 201)
    assert (std["T"][std["isrc"]] + std["T"][std["irec"]]).max() < K.NT * K.DT
    img, cnt = K.migrate(std["T"], std["isrc"], std["irec"], std["data"], K.DT)
    iy, ix = np.unravel_index(np.argmax(np.abs(img[0])), img[0].shape)
    peak = img[0, K.SCATTERER[1], K.SCATTERER[0]] / N
    print(f"peak at {(ix, iy)}, I / N there {peak:.5f}, contributing {cnt}")
    assert (ix, iy) == K.SCATTERER
    assert 0.98 <= peak <= 1.0
    assert cnt == N * 201 * 101

    bins, cntb = K.migrate(std["T"], std["isrc"], std["irec"], std["data"], K.DT, theta=std["theta"], nbin=K.NBIN, dopen=K.DOPEN)
    h = K.half_opening(std["theta"], std["isrc"], std["irec"])
    share = np.bincount(np.floor(h / K.DOPEN).astype(int), minlength=K.NBIN) / N
    got = bins[:, K.SCATTERER[1], K.SCATTERER[0]] / N
    print("traces per bin", (share * N).astype(int), "image / N per bin", np.round(got, 4))
    assert list((share * N).round().astype(int)) == [215, 137, 111, 88, 25, 0]
    assert np.all(np.abs(got - share) <= 0.02)
    e = np.max(np.abs(bins.sum(axis=0) - img[0])) / np.max(np.abs(img))
    print(f"sum of bins against the unbinned image: {e:.2e}")
    assert cntb == cnt and e <= 1e-12


@pytest.mark.parametrize("nbin", [0, 6])
@pytest.mark.parametrize("holes", [False, True])
def test_adjointness_of_the_restatement(std, nbin, holes):
    rng = np.random.default_rng(7 + nbin + holes)
    T, th = std["T"], std["theta"]
    amp = 0.5 + rng.random(T.shape)
    if holes:
        T, th, amp = K.with_holes(T, rng), K.with_holes(th, rng), K.with_holes(amp, rng)
    w = rng.standard_normal(len(std["isrc"]))
    kw = dict(amp=amp, theta=th if nbin else None, w=w, nbin=nbin, dopen=K.DOPEN if nbin else None)
    d = rng.standard_normal((len(w), K.NT))
    m = rng.standard_normal((max(nbin, 1),) + T.shape[1:])
    L = K.matrix(T, std["isrc"], std["irec"], K.NT, K.DT, **kw)
    img, cnt = K.migrate(T, std["isrc"], std["irec"], d, K.DT, **kw)
    assert L.nnz == 2 * cnt
    Lm = L @ m.reshape(-1)
    lhs, rhs = float(Lm @ d.reshape(-1)), float(m.reshape(-1) @ img.reshape(-1))
    scale = float(np.abs(d.reshape(-1)) @ (abs(L) @ np.abs(m.reshape(-1))))            # the sum of |terms|
    print(f"nbin {nbin} holes {holes}: <Lm, d> {lhs:.12e} <m, L^T d> {rhs:.12e}, |diff| / sum|terms| {abs(lhs - rhs) / scale:.2e}, "
          f"contributing {cnt} of {len(w) * T[0].size}")
    assert abs(lhs - rhs) <= 1e-13 * scale
    if holes:
        assert cnt < 0.95 * len(w) * T[0].size
    # L^T as the matrix transpose: the loop and the matrix hold the same weights
    assert np.max(np.abs(L.T @ d.reshape(-1) - img.reshape(-1))) <= 1e-12 * np.max(np.abs(img))


def test_lsqr_on_the_restatement(std):
    from scipy.sparse.linalg import lsqr
    L = K.matrix(std["T"], std["isrc"], std["irec"], K.NT, K.DT)
    d = L @ K.lsm_model().reshape(-1)
    ratios = [float(np.linalg.norm(L @ lsqr(L, d, atol=0, btol=0, iter_lim=it)[0] - d) / np.linalg.norm(d)) for it in (5, 10, 20)]
    print("LSQR residual ratios after 5, 10, 20 iterations:", np.round(ratios, 4))
    assert ratios[0] > ratios[1] > ratios[2] and ratios[1] < 0.3
