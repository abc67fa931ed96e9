"""GPU: location pdfs (rtmi_locate_pdf, rtmi_locate_edt_pdf and their _dev forms).  Every output is
compared with the restatement tests/pdf_ref.py on the maps of tests/locate_ref.py and tests/edt_ref.py, bit for bit: the density
is one text on both sides, the masses are integers, every sum over them is an integer sum, and the per-event results are host
arithmetic.  The shapes are the smallest at which the kernels can go wrong: one full tile, 255 nodes, 257 nodes in one row (two
tiles, and the rim is everything), five tiles with a partial last one; 2, 3, 7 and 33 stations; 1, 16, 17 and 35 events; both
kinds with and without weights; one tile per block, so that an event's sums come from several blocks' atomics."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import edt_ref
import locate_ref
import pdf_ref
from test_gpu_edt import problem
from test_pdf_host import struct_sizes_match_gccs

pytestmark = pytest.mark.gpu

LEVELS = (0.5, 0.68, 0.95, 0.999)
PDF_KEYS = ("mean_x", "mean_y", "pdf_cov", "ellipse", "area", "rim_fraction", "nz", "mass", "level_count", "level_area",
            "level_fraction", "level_rho")
L2_SIGMA, L2_SIGMA_W, EDT_SIGMA, EDT_SIGMA_W = 0.1, 3.0, 0.05, 0.01


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = C.c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def uniforms(E, S, seed=1):
    """[E, S] in [0, 1) with 0 and the greatest double below 1 in every row that has room for them"""
    u = np.random.default_rng(seed).random((E, S))
    if S >= 1:
        u[::2, 0] = 0.0
        u[1::2, 0] = np.nextafter(1.0, 0.0)
    if S >= 2:
        u[:, 1] = np.where(np.arange(E) % 2 == 0, np.nextafter(1.0, 0.0), 0.0)
    return u


_searched = {}


def searched(kind, grid, T, t, sigma, w, need):
    """the restated search of a problem, computed once per module"""
    h = hashlib.sha1()
    for a in (T, t, w, need):
        h.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
    key = (kind, tuple(grid), float(sigma) if kind == "edt" else None, h.hexdigest())
    if key not in _searched:
        _searched[key] = (locate_ref.locate(T, t, w=w, need=need, grid=grid) if kind == "l2"
                          else edt_ref.locate(T, t, sigma, w=w, need=need, grid=grid))
    return _searched[key]


def same(got, want, keys, what=""):
    for k in keys:
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k, got[k], want[k])


def expected(kind, grid, T, t, sigma, w=None, need=None, power=0, levels=LEVELS, u=None):
    best = searched(kind, grid, T, t, sigma, w, need)
    params = dict(kind=kind, sigma=sigma, power=power, levels=levels, u=u, marginals=True)
    return best, pdf_ref.pdf(best["maps"], best, params, grid)


def run(L, kind, t, sigma, w=None, need=None, power=0, levels=LEVELS, u=None, **kw):
    S = 0 if u is None else u.shape[1]
    return L.pdf(t, sigma, method=kind, weights=w, min_picks=need, power=power, levels=levels, marginals=True, samples=S, u=u,
                 stats=True, **kw)


def check(rb, kind, grid, T, t, sigma, w=None, need=None, power=0, levels=LEVELS, S=300, what="", **kw):
    """the host entry against the restatement, everything it returns; and res against the plain search's result"""
    E = len(t)
    u = uniforms(E, S) if S else None
    best, want = expected(kind, grid, T, t, sigma, w, need, power, levels, u)
    L = rb.Locator(T, grid)
    try:
        got, st = run(L, kind, t, sigma, w, need, power, levels, u, **kw)
        plain = L.locate(t, weights=w, min_picks=need) if kind == "l2" else L.locate_edt(t, sigma, weights=w, min_picks=need)
    finally:
        L.close()
    same(got, plain, plain.keys(), what + ": res against the plain search")
    assert np.array_equal(got["node"], best["node"]), what
    same(got, want, PDF_KEYS + ("mx", "my"), what)
    if S:
        same(got, want, ("sample_node",), what)
        has = want["mass"] > 0
        assert (got["sample_node"][has] >= 0).all() and (got["sample_node"][~has] == -1).all()
    else:
        assert "sample_node" not in got
    assert got["level_count"].shape == (E, len(levels))
    return got, want, st


def test_struct_sizes_match_gccs(tmp_path):
    struct_sizes_match_gccs(tmp_path)


# ---------------------------------------------------------------- 1. shapes
SHAPES = [  # kind, nx, ny, P, E: every grid, every P and every E of the list above at least once per kind
    ("l2", 16, 16, 2, 1), ("l2", 16, 16, 7, 17), ("l2", 17, 15, 3, 16), ("l2", 257, 1, 7, 35), ("l2", 37, 29, 33, 35), ("l2", 37, 29, 3, 17),
    ("edt", 16, 16, 2, 1), ("edt", 16, 16, 7, 17), ("edt", 17, 15, 3, 16), ("edt", 17, 15, 33, 1), ("edt", 257, 1, 7, 35), ("edt", 37, 29, 7, 35),
]


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("kind,nx,ny,P,E", SHAPES)
def test_every_output_has_the_restatements_bits(rb, kind, nx, ny, P, E, weights):
    grid, T, t, w = problem(nx, ny, P, E, seed=nx + 7 * ny + 13 * P + E, weights=weights)
    sigma = {("l2", False): L2_SIGMA, ("l2", True): L2_SIGMA_W, ("edt", False): EDT_SIGMA, ("edt", True): EDT_SIGMA_W}[kind, weights]
    got, want, st = check(rb, kind, grid, T, t, sigma, w, _tiles_per_block=1)
    assert (got["mass"] >= pdf_ref.ONE).all() and (got["nz"] >= 1).all() and st["groups"] == 1
    assert np.isfinite(got["mean_x"]).all() and (got["level_fraction"] >= np.array(LEVELS)).all()
    assert np.allclose(got["mx"].sum(axis=1), 1.0, rtol=0, atol=1e-12) and np.allclose(got["my"].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    if ny == 1:
        assert (got["rim_fraction"] == 1.0).all()
    if nx * ny > 256 and P >= 7:
        assert (got["nz"] > 1).any()                              # a pdf of several nodes: the moments are not all zero
    # the default run of 64 tiles per block: the same bits from one block per event
    L = rb.Locator(T, grid)
    again, _ = run(L, kind, t, sigma, w, None, 0, LEVELS, uniforms(E, 300))
    L.close()
    same(again, got, PDF_KEYS + ("mx", "my", "sample_node"), "64 tiles per block")


@pytest.mark.parametrize("power", [0, 1, 13])
def test_edt_powers(rb, power):
    grid, T, t, w = problem(37, 29, 7, 17, seed=40)
    got, want, _ = check(rb, "edt", grid, T, t, EDT_SIGMA, power=power, S=1, _tiles_per_block=2)
    assert (got["mass"] > pdf_ref.ONE).all()


def test_powers_order_the_areas(rb):
    grid, T, t, w = problem(37, 29, 7, 17, seed=40)
    L = rb.Locator(T, grid)
    area = [L.pdf(t, EDT_SIGMA, method="edt", power=p, levels=())["area"] for p in (1, 7, 0, 13)]
    L.close()
    assert np.array_equal(area[1], area[2])                       # power 0 is the number of readings: 7
    assert (area[0] > area[1]).all() and (area[1] > area[3]).all()


@pytest.mark.parametrize("kind", ["l2", "edt"])
def test_no_levels_no_samples_no_marginals(rb, kind):
    grid, T, t, w = problem(37, 29, 7, 17, seed=41)
    sigma = L2_SIGMA if kind == "l2" else EDT_SIGMA
    got, want, _ = check(rb, kind, grid, T, t, sigma, levels=(), S=0)
    L = rb.Locator(T, grid)
    bare = L.pdf(t, sigma, method=kind, levels=())
    one = L.pdf(t, sigma, method=kind, levels=(0.9,), samples=5, seed=3)
    two = L.pdf(t, sigma, method=kind, levels=(0.9,), samples=5, seed=3, jitter=False)
    L.close()
    same(bare, got, PDF_KEYS, "without marginals")
    assert "mx" not in bare and "sample_node" not in bare and bare["level_rho"].shape == (17, 0)
    # the seeded draw: numpy.random.default_rng(seed), the same nodes with and without the offset within the cell
    assert np.array_equal(one["sample_u"], np.random.default_rng(3).random((17, 5)))
    assert np.array_equal(one["sample_node"], two["sample_node"])
    assert np.array_equal(two["sample_x"], grid[0] + (two["sample_node"] % 37) * grid[1])
    assert (np.abs(one["sample_x"] - two["sample_x"]) <= 0.5 * grid[1]).all() and (one["sample_x"] != two["sample_x"]).any()
    assert (np.abs(one["sample_y"] - two["sample_y"]) <= 0.5 * grid[4]).all()


# ---------------------------------------------------------------- 2. holes, events without a pdf, rims
@pytest.mark.parametrize("kind", ["l2", "edt"])
def test_tables_with_holes_and_an_event_with_no_candidate_beside_good_ones(rb, kind):
    P, E = 7, 17
    grid, T, t, w = problem(37, 29, P, E, seed=42, holes=0.05, weights=True)
    t[3] = np.nan                                                 # no pick at all
    t[9, 1:] = np.nan                                             # one pick: need cannot be met
    need = np.full(E, P - 2, dtype=np.int32)
    need[12] = P + 1                                              # a need above P: no candidate
    sigma = L2_SIGMA_W if kind == "l2" else EDT_SIGMA_W
    got, want, _ = check(rb, kind, grid, T, t, sigma, w, need, _tiles_per_block=1)
    none = np.zeros(E, dtype=bool)
    none[[3, 9, 12]] = True
    assert (got["node"][none] == -1).all() and (got["node"][~none] >= 0).all()
    assert (got["mass"][none] == 0).all() and (got["nz"][none] == 0).all() and (got["level_count"][none] == 0).all()
    for k in ("mean_x", "mean_y", "pdf_cov", "ellipse", "area", "rim_fraction", "level_area", "level_fraction", "level_rho", "mx", "my"):
        assert np.isnan(got[k][none]).all() and np.isfinite(got[k][~none]).all(), k
    assert (got["sample_node"][none] == -1).all()
    assert (want["m"][~none].reshape(14, -1) == 0).any(axis=1).all()          # nodes that are no candidates: no mass


def test_an_edt_event_whose_every_pair_is_cut_has_no_pdf(rb):
    P, E = 7, 17
    grid, T, t, _ = problem(37, 29, P, E, seed=6, noise=0.002)
    t[16] = 100.0 * np.arange(P)                                  # value = 0 at every node: the best node is node 0
    got, want, _ = check(rb, "edt", grid, T, t, 0.01)
    assert got["node"][16] == 0 and got["value"][16] == 0.0 and got["mass"][16] == 0 and np.isnan(got["area"][16])
    assert (got["sample_node"][16] == -1).all() and np.isnan(got["mx"][16]).all() and (got["mass"][:16] > 0).all()


@pytest.mark.parametrize("kind", ["l2", "edt"])
def test_best_node_on_each_rim_and_in_a_corner(rb, kind):
    nx, ny = 37, 29
    grid, T, _, _ = problem(nx, ny, 7, 1, seed=10)
    nodes = [(0, 12), (nx - 1, 12), (17, 0), (17, ny - 1), (0, 0), (nx - 1, ny - 1), (0, ny - 1), (nx - 1, 0), (17, 12)]
    t = np.stack([4.0 + T[:, iy, ix] for ix, iy in nodes])
    got, want, _ = check(rb, kind, grid, T, t, L2_SIGMA if kind == "l2" else 0.02, _tiles_per_block=2)
    for e, (ix, iy) in enumerate(nodes):
        assert (got["ix"][e], got["iy"][e]) == (ix, iy)
    assert (got["rim_fraction"][:8] > 0.2).all() and got["rim_fraction"][8] < got["rim_fraction"][:8].min()
    # the mean of a pdf cut off by the rim lies inside the grid, away from the best node
    assert got["mean_x"][0] > grid[0] and got["mean_y"][2] > grid[3]
    # a tight density in the interior: nothing on the rim, exactly.  An EDT value does not fall to 0 far from the best node (the
    # pairs that do not resolve the move keep their kernels), so there it is the power that makes the density tight
    L = rb.Locator(T, grid)
    tight = L.pdf(t[8:], 0.02, method=kind, power=0 if kind == "l2" else 256, levels=())
    L.close()
    assert tight["rim_fraction"][0] == 0.0 and tight["mass"][0] > 0


# ---------------------------------------------------------------- 3. groups, device pointers, splits
@pytest.mark.parametrize("kind,weights", [("l2", False), ("l2", True), ("edt", False), ("edt", True)])
def test_groups_device_pointers_and_the_split_of_a_call(rb, torch, kind, weights):
    P, E = 7, 35
    grid, T, t, w = problem(37, 29, P, E, seed=43, holes=0.03, weights=weights)
    t[20, [1, 4]] = np.nan
    t[21] = np.nan
    need = np.full(E, P - 2, dtype=np.int32)
    sigma = {("l2", False): L2_SIGMA, ("l2", True): L2_SIGMA_W, ("edt", False): EDT_SIGMA, ("edt", True): EDT_SIGMA_W}[kind, weights]
    u = uniforms(E, 300)
    every = PDF_KEYS + ("mx", "my", "sample_node")
    _, want = expected(kind, grid, T, t, sigma, w, need, 0, LEVELS, u)
    L = rb.Locator(T, grid)
    one, st = run(L, kind, t, sigma, w, need, 0, LEVELS, u)
    assert st["groups"] == 1 and st["pdf_ms"] > 0.0 and st["kernel_ms"] > st["pdf_ms"]
    same(one, want, every, "one group")
    search_keys = tuple(k for k in one if k not in every + ("sample_x", "sample_y", "sample_u"))
    for per, groups in ((1, 35), (3, 12), (16, 3), (64, 1)):
        many, st = run(L, kind, t, sigma, w, need, 0, LEVELS, u, _events_per_group=per, _tiles_per_block=1 + per % 2)
        assert st["groups"] == groups
        same(many, one, every + search_keys, f"{per} events per group")
    # device pointers
    dev = "cuda:0"
    tt = lambda a: None if a is None else torch.from_numpy(a).to(dev)          # noqa: E731
    d, dst = L.pdf_device(tt(t), sigma, method=kind, weights=tt(w), min_picks=tt(need), levels=LEVELS, marginals=True, samples=300, u=tt(u),
                          stats=True, _events_per_group=16)
    assert dst["groups"] == 3
    for k in ("mx", "my", "sample_node"):
        assert d[k].is_cuda
        d[k] = d[k].cpu().numpy()
    same(d, one, every + search_keys, "pdf_device")
    seeded = L.pdf_device(tt(t), sigma, method=kind, weights=tt(w), min_picks=tt(need), samples=4, seed=5)
    assert np.array_equal(seeded["sample_u"].cpu().numpy(), np.random.default_rng(5).random((E, 4)))
    with pytest.raises(ValueError, match="on a GPU"):
        L.pdf_device(torch.from_numpy(t), sigma, method=kind)
    # a call split 20 + 15
    parts = [run(L, kind, t[a:b], sigma, None if w is None else w[a:b], need[a:b], 0, LEVELS, u[a:b])[0] for a, b in ((0, 20), (20, 35))]
    for k in every + search_keys:
        assert np.array_equal(np.concatenate([p[k] for p in parts]), one[k], equal_nan=True), k
    L.close()


# ---------------------------------------------------------------- 4. refusals
def test_refusals_name_the_argument_and_the_handle_stays_usable(rb):
    from raytracing_amd import _lib
    grid, T, t, w = problem(16, 16, 3, 5, seed=44, weights=True)
    L = rb.Locator(T, grid)
    lib = _lib.lib()
    pdf = (_lib.PdfResult * 5)()
    u, sm = np.full((5, 2), 0.5), np.zeros((5, 2), dtype=np.int32)

    def params(**kw):
        pp = _lib.PdfParams()
        pp.sigma, pp.nlevels = 0.1, 1
        pp.levels[0] = 0.5
        for k, v in kw.items():
            if k == "level":
                pp.levels[0] = v
            elif k.startswith("reserved"):
                pp.reserved[int(k[-1])] = v
            else:
                setattr(pp, k, v)
        return pp

    def l2(pp, pdf=pdf, u=None, samples=None, need=None):
        return lib.rtmi_locate_pdf(L._h, None if pp is None else C.byref(pp), 5, _lib.dptr(t), None,
                                   None if need is None else need.ctypes.data_as(_lib._ip), None, pdf, None, None, _lib.dptr(u),
                                   None if samples is None else samples.ctypes.data_as(_lib._ip), None)

    def edt(pp, sigma=0.05, ep=True, weights=None, group=0):
        e = _lib.EdtParams()
        e.sigma = sigma
        e.reserved[0] = group
        return lib.rtmi_locate_edt_pdf(L._h, C.byref(e) if ep else None, None if pp is None else C.byref(pp), 5, _lib.dptr(t),
                                       _lib.dptr(weights), None, None, pdf, None, None, None, None, None)

    def refused(rc, who, *words):
        msg = lib.rtmi_last_error()
        assert rc == -1 and msg.startswith(who.encode() + b": "), msg
        for word in words:
            assert word.encode() in msg, msg

    who = "rtmi_locate_pdf"
    refused(l2(None), who, "null pp")
    refused(l2(params(), pdf=None), who, "null pdf")
    for n in (-1, 9):
        refused(l2(params(nlevels=n)), who, "nlevels must be in 0 .. 8")
    for c in (0.0, 1.0, -0.5, 1.5, np.nan):
        refused(l2(params(level=c)), who, "levels[0] is not in (0, 1)")
    refused(l2(params(S=-1)), who, "S must be >= 0")
    refused(l2(params(S=2), u=None, samples=sm), who, "null u or samples")
    refused(l2(params(S=2), u=u, samples=None), who, "null u or samples")
    for p in (-1, 4097):
        refused(l2(params(power=p)), who, "power must be in 0 .. 4096")
    for s in (0.0, -0.1, np.nan, np.inf):
        refused(l2(params(sigma=s)), who, "sigma must be finite and > 0")
    refused(l2(params(reserved0=-1)), who, "reserved[0]")
    refused(l2(params(reserved1=-1)), who, "reserved[0] and reserved[1]")
    refused(l2(params(), need=np.array([1, 1, -1, 1, 1], dtype=np.int32)), who, "need[2] is negative")
    who = "rtmi_locate_edt_pdf"
    refused(edt(None), who, "null pp")
    refused(edt(params(), ep=False), who, "null ep")
    for s in (0.0, -0.1, np.nan, np.inf):
        refused(edt(params(), sigma=s), who, "ep->sigma must be finite and > 0")
    for s in (-0.1, np.nan, np.inf):
        refused(edt(params(), sigma=s, weights=w), who, "ep->sigma must be finite and >= 0")
    refused(edt(params(), group=-1), who, "ep->reserved[0] must be >= 0")
    refused(edt(params(power=4097)), who, "power must be in 0 .. 4096")
    assert edt(params(sigma=np.nan)) == 0                         # pp->sigma is not read by the EDT kind
    # through Python, and both _dev entries: a host pointer is refused by name
    with pytest.raises(_lib.RtmiError, match=r"rtmi_locate_pdf: levels\[1\] is not in \(0, 1\)"):
        L.pdf(t, 0.1, levels=(0.5, 1.0))
    pp = params()
    rc = lib.rtmi_locate_pdf_dev(L._h, C.byref(pp), 5, t.ctypes.data, None, None, None, pdf, None, None, None, None, None)
    refused(rc, "rtmi_locate_pdf_dev", "d_t is not memory of the handle's device")
    e = _lib.EdtParams()
    e.sigma = 0.05
    rc = lib.rtmi_locate_edt_pdf_dev(L._h, C.byref(e), C.byref(pp), 5, t.ctypes.data, None, None, None, pdf, None, None, None, None, None)
    refused(rc, "rtmi_locate_edt_pdf_dev", "d_t is not memory of the handle's device")
    # the handle is usable afterwards
    assert (L.pdf(t, 0.1)["mass"] > 0).all() and (L.pdf(t, 0.05, method="edt")["mass"] > 0).all()
    L.close()
    with pytest.raises(RuntimeError, match="closed"):
        L.pdf(t, 0.1)
    # an axis above 65 536 nodes
    wide = rb.Locator(np.zeros((1, 1, 65537)), (0.0, 1.0, 65537, 0.0, 1.0, 1))
    with pytest.raises(_lib.RtmiError, match="rtmi_locate_pdf: nx or ny is over 65536"):
        wide.pdf(np.zeros((1, 1)), 0.1)
    assert wide.locate(np.zeros((1, 1)))["node"][0] == 0
    wide.close()


def test_an_axis_of_65536_nodes(rb):
    """the widest axis the entries take: a flat map along it, so that Sxx is 2^30 times the sum of di^2 over 65 536 nodes, past
    2^77, and the two-word sums and their conversion are at work"""
    nx = 65536
    T = np.zeros((1, 1, nx))
    grid = (0.0, 1.0, nx, 0.0, 1.0, 1)
    t = np.array([[1.0]])
    L = rb.Locator(T, grid)
    u = np.array([[0.0, 0.5, np.nextafter(1.0, 0.0)]])
    got, st = L.pdf(t, 1.0, levels=(0.5,), marginals=True, samples=3, u=u, stats=True)
    L.close()
    assert got["node"][0] == 0 and got["mass"][0] == nx << 30 and got["nz"][0] == nx and got["rim_fraction"][0] == 1.0
    sxx = (nx - 1) * nx * (2 * nx - 1) // 6
    ax = float((nx - 1) * nx // 2 << 30) / float(nx << 30)
    assert got["mean_x"][0] == (0.0 + 0.0 * 1.0) + ax * 1.0 == (nx - 1) / 2
    assert got["pdf_cov"][0, 0, 0] == (float(sxx << 30) / float(nx << 30) - ax * ax) * (1.0 * 1.0)
    assert got["sample_node"][0].tolist() == [0, nx // 2, nx - 1]
    assert np.array_equal(got["mx"][0], np.full(nx, 1.0 / nx)) and got["level_count"][0, 0] == nx
