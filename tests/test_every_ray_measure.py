"""The per-ray comparator of tests/every_ray.py (what tests/test_gpu_every_ray.py judges whole fans with) against bench.py's
batch-wide measures, on seeded synthetic arrays in every layout the tests compare: no GPU needed."""
import numpy as np
import pytest
import torch

from bench import QUANTITY_GROUPS, parity_relerr, parity_relerr_elementwise
from every_ray import fingerprint, group_scales, offenders, per_ray_error, worst

R = 1000                     # no power of two: the chunk sizes below leave a short last chunk


def synthetic(layout, seed):
    """(a, b): b a plausible batch of the layout, a = b moved by a few ulps-ish relative noise."""
    rng = np.random.default_rng(seed)
    shape = {"final": (9, R), "rows": (37, 6, R), "d_ray": (3, R)}[layout]
    # quantities of very different magnitude, as in a batch: x ~ 5, p ~ 0.05, T ~ 0.4, step counts ~ 1e3
    mag = {9: [5, 5, 1.5, 1.4, 1e-3, 1e-3, 0.05, 0.05, 0.4], 6: [5, 5, 0.05, 0.05, 0.4, 1.5], 3: [80, 80, 3000]}[shape[-2]]
    b = rng.standard_normal(shape) * np.array(mag)[:, None]
    a = b * (1 + 1e-13 * rng.standard_normal(shape)) + 1e-15 * rng.standard_normal(shape)
    return a, b


def reference(a, b):
    return max(parity_relerr(a, b), parity_relerr_elementwise(a, b))


@pytest.mark.parametrize("layout", ["final", "rows", "d_ray"])
@pytest.mark.parametrize("chunk", [None, 96, 333])
def test_max_over_rays_is_bench_measure_bit_for_bit(layout, chunk):
    a, b = synthetic(layout, 1)
    err, _ = per_ray_error(a, b, chunk=chunk)
    assert err.shape == (R,) and err.dtype == torch.float64
    assert float(err.max()) == reference(a, b) > 0
    # ... and on torch tensors, the same bits
    err_t, _ = per_ray_error(torch.from_numpy(a), torch.from_numpy(b), chunk=chunk)
    assert torch.equal(err, err_t)


def test_grad_n_floor():
    """Every end point in a constant part of the medium: grad n ~ 1e-40, its scale floored at the index's (bench.parity_relerr)."""
    a, b = synthetic("final", 2)
    b[4:6] *= 1e-40
    a[4:6] = b[4:6] * 3.0                             # relative error 2 against its own scale: only the floor makes it tiny
    a[4, 17] = b[4, 17] + 3e-9 * np.abs(b[3]).max()   # one ray's gradient off by 3e-9 of the index's scale
    err, grp = per_ray_error(a, b, chunk=128)
    assert float(err.max()) == reference(a, b)
    assert worst(err, 1)[0] == 17 and int(grp[17]) == 3
    assert list(offenders(err, 1e-9)) == [17]
    assert group_scales(b)[3] == np.abs(b[3]).max() > np.abs(b[4:6]).max()


@pytest.mark.parametrize("layout", ["final", "rows", "d_ray"])
def test_planted_error_and_nan_come_back_as_their_rays(layout):
    a, b = synthetic(layout, 3)
    Q = b.shape[-2]
    q = {9: 8, 6: 2, 3: 0}[Q]                         # T; p_x of a row; dist_real
    gi = [i for i, g in enumerate(QUANTITY_GROUPS[Q]) if q in g][0]
    scale = group_scales(b)[gi]
    # the planted value sits at the group's largest magnitude, so that both measures read it as 2e-9
    if a.ndim == 3:
        b[20, q, 411] = scale                         # one row of one ray
    else:
        b[q, 411] = scale
    a[..., q, 411] = b[..., q, 411]
    if a.ndim == 3:
        a[20, q, 411] = scale + 2e-9 * scale
    else:
        a[q, 411] = scale + 2e-9 * scale
    a[..., 1, 640] = np.nan                           # another ray: NaN in one quantity
    for chunk in (None, 96, 333):
        err, grp = per_ray_error(a, b, chunk=chunk)
        assert float(err[640]) == np.inf
        assert 2e-9 * (1 - 1e-6) < float(err[411]) < 2e-9 * (1 + 1e-6) and int(grp[411]) == gi
        assert list(offenders(err, 1e-9)) == [411, 640]
        assert list(worst(err, 2)) == [640, 411]
    # a NaN on the reference's side counts too, and does not poison the other rays through the scale
    a2, b2 = synthetic(layout, 4)
    b2[..., 0, 5] = np.nan
    err, _ = per_ray_error(a2, b2, chunk=333)
    assert list(offenders(err, 1e-9)) == [5]


def test_offenders_never_let_a_nan_through():
    """offenders() on per-ray errors that still hold a NaN (e.g. computed elsewhere): ~(err <= tol), not err > tol."""
    err = torch.tensor([0.0, np.nan, 2e-9, 1e-9, np.inf, 5e-10], dtype=torch.float64)
    assert list(offenders(err, 1e-9)) == [1, 2, 4]
    assert list(offenders(err.numpy(), 1e-9)) == [1, 2, 4]


def test_chunked_equals_unchunked_everywhere():
    a, b = synthetic("rows", 5)
    a[3, 0, 7] = np.nan
    e0, g0 = per_ray_error(a, b)
    for chunk in (1, 7, 96, 999, 1000, 4096):
        e, g = per_ray_error(a, b, chunk=chunk)
        assert torch.equal(e, e0) and torch.equal(g, g0)


def test_fingerprint_is_exact_per_ray():
    a, b = synthetic("rows", 6)
    f = fingerprint(b, chunk=333)
    assert f.shape == (6, R) and f.dtype == torch.int64
    assert torch.equal(f, fingerprint(torch.from_numpy(b.copy())))
    # wrap-around int64 sum of each ray's bits per quantity
    want = b.view(np.int64).sum(axis=0)
    assert np.array_equal(f.numpy(), want)
    c = b.copy()
    c[30, 4, 123] = np.nextafter(c[30, 4, 123], np.inf)         # one ulp of one row of one ray
    diff = (fingerprint(c, chunk=96) != f).nonzero().tolist()
    assert diff == [[4, 123]]
    f32 = fingerprint(b.astype(np.float32))
    assert f32.shape == (6, R) and torch.equal(f32, torch.from_numpy(b.astype(np.float32).view(np.int32).astype(np.int64).sum(axis=0)))
