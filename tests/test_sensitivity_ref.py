"""CPU: the numpy restatement of the traveltime sensitivity kernels (tests/sensitivity_ref.py) on the oracle's rows: A Z gives
back the recorded traveltimes at the ray ends and at the crossings, A 1 the chord sum, the restatement is its own adjoint, and
the path-fixed derivative matches central differences of re-traced rays in perturbed fields (Fermat).  No GPU involved; these
validate the restatement before the device is compared with it (tests/test_gpu_sensitivity.py)."""
import numpy as np
import pytest

import crossing_ref as X
import sensitivity_ref as S
from conftest import LIMITS

SIGMA = 0.05293304824724534
DELTA = SIGMA / 3
DELTA_S = SIGMA / 20

# scenario -> (step, launch point, fan, line)
SCEN = {
    "interface": (DELTA_S, (-2.0, -2.0), (2 * np.pi / 60, np.pi / 2), (0.0, 1.0, 1.0)),
    "fisheye": (2 * np.pi / 303, (1.0, 0.0), (np.pi / 2 - 0.4, np.pi / 2 + 0.4), (0.0, 1.0, 0.3)),
    "vert_heterogeneous": (DELTA_S, (-2.0, -2.0), (0.05, np.pi / 2 - 0.05), (1.0, 0.0, 2.0)),
    "anisotropy": (DELTA_S, (-2.0, -2.0), (0.05, np.pi / 2 - 0.05), (1.0, 0.0, 2.0)),
}
_FIELDS = {}


def field(scen):
    from oracle import rt_oracle as O
    if scen not in _FIELDS:
        _FIELDS[scen] = O.Field(scen, LIMITS[scen], DELTA)
    return _FIELDS[scen]


def trace(F, scen, m, R, gamma=1.0):
    from oracle import rt_oracle as O
    step, (x0, y0), fan, _ = SCEN[scen]
    ms = 10 * 304 if scen == "fisheye" else int(np.ceil(80 / step) + 1)
    th = np.linspace(*fan, R)
    c = O.trazar(F, m, gamma, step, ms, LIMITS[scen], x0, y0, th, record_stride=0, nthreads=8)
    rows = int(c["d_ray"][2].max()) + 1
    o = O.trazar(F, m, gamma, step, ms, LIMITS[scen], x0, y0, th, record_stride=1, rec_rows=rows, nthreads=8)
    return o


def rel(a, b):
    ok = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), ok)
    return float(np.max(np.abs(a[ok] - b[ok])) / np.max(np.abs(b[ok])))


CASES = [(s, m) for s in ("interface", "fisheye", "vert_heterogeneous") for m in range(1, 10)] + \
        [("anisotropy", 10), ("anisotropy", 11)]


@pytest.mark.parametrize("scen,m", CASES)
def test_A_Z_gives_back_the_recorded_traveltimes(scen, m):
    F = field(scen)
    gamma = 3.0 if scen == "anisotropy" else 1.0
    o = trace(F, scen, m, 12, gamma)
    s, last = o["s_ray"], o["d_ray"][2].astype(np.int64)
    x, y, Z = F.arrays()[:3]
    ax, ay = S.axes(x, y)
    line = SCEN[scen][3]
    M = S.matrices(s, last, ax, ay, line=line, kmax=4, method=m, gamma=gamma)
    d = S.perturb(M, Z)
    R = s.shape[2]
    assert rel(d["end"], s[last, 4, np.arange(R)]) <= 1e-12
    assert np.any(M["count"] > 0)
    assert rel(d["line"], M["crossings"][:, 3]) <= 1e-12
    if m < 10:
        assert rel(S.perturb(M, np.ones_like(Z))["end"], o["d_ray"][1]) <= 1e-12       # the chord sum


def test_restatement_is_its_own_adjoint():
    F = field("vert_heterogeneous")
    o = trace(F, "vert_heterogeneous", 6, 16)
    x, y, Z = F.arrays()[:3]
    ax, ay = S.axes(x, y)
    M = S.matrices(o["s_ray"], o["d_ray"][2], ax, ay, line=SCEN["vert_heterogeneous"][3], kmax=3)
    rng = np.random.default_rng(3)
    dz = rng.standard_normal(Z.shape)
    d = S.perturb(M, dz)
    we = rng.standard_normal(16)
    wl = np.where(np.isfinite(d["line"]), rng.standard_normal(d["line"].shape), np.nan)
    lhs = np.dot(d["end"], we) + np.nansum(d["line"] * wl)
    rhs = np.dot(dz.ravel(), S.backproject(M, we, wl))
    assert abs(lhs - rhs) <= 1e-13 * max(abs(lhs), np.sum(np.abs(d["end"] * we)))


def bump(x, y, cx, cy, w):
    X_, Y_ = np.meshgrid(x, y)
    return np.exp(-((X_ - cx) ** 2 + (Y_ - cy) ** 2) / (2 * w * w))


@pytest.mark.parametrize("scen,centre", [("vert_heterogeneous", (0.5, -1.0)), ("fisheye", (0.3, 0.1))])
def test_fermat_central_difference(scen, centre):
    """The crossing T of re-traced rays in Z +- eps dZ, moved back to the unperturbed crossing point along the line with the
    slowness along it, against A dZ (first crossings present in all three traces)."""
    from oracle import rt_oracle as O
    F = field(scen)
    x, y, Z = F.arrays()[:3]
    ax, ay = S.axes(x, y)
    line = SCEN[scen][3]
    a, b, c = X.normalise(line)
    dz = bump(x, y, *centre, 0.4) * Z
    eps = 1e-4
    R = 24
    o = trace(F, scen, 6, R)
    M = S.matrices(o["s_ray"], o["d_ray"][2], ax, ay, line=line, kmax=1)
    ad = S.perturb(M, dz)["line"][0]
    cr0 = M["crossings"][0]
    Ts = []
    for sgn in (1.0, -1.0):
        Fp = O.Field.from_samples(x, y, Z + sgn * eps * dz, DELTA)
        op = trace(Fp, scen, 6, R)
        cnt, cr = X.crossings(op["s_ray"], op["d_ray"][2], line, kmax=1)
        u, T, th = cr[0, 0], cr[0, 3], cr[0, 4]
        n = Fp.n_gradient(cr[0, 1], cr[0, 2])[0]
        dTdu = n * (np.cos(th) * -b + np.sin(th) * a)
        Ts.append(T + (cr0[0] - u) * dTdu)
    fd = (Ts[0] - Ts[1]) / (2 * eps)
    ok = np.isfinite(fd) & np.isfinite(ad)
    assert ok.sum() >= 8
    err = np.max(np.abs(fd[ok] - ad[ok])) / np.max(np.abs(ad[ok]))
    print(f"{scen}: Fermat central difference vs A dZ {err:.2e} over {ok.sum()} rays")
    assert err <= 1e-3                   # measured 2.1e-4 (vert_heterogeneous), 1.7e-4 (fisheye): DESIGN.md 12
