"""GPU: runs continued from a caller-set ray state (rtmi_batch_set_state) against the oracle's continuation of the same states
(oracle.rt_oracle.trazar_from_state).

The states lie off the batch's own launch trajectories: they are oracle rows perturbed (x by 1e-3, theta by 1e-4, n and its
gradient taken at the new point), and every batch is launched from conditions unrelated to them (theta = pi/4 from (-2, -2)).
A run that fell back to the launch conditions anywhere -- the automatic re-trace of critical rays included -- cannot give the
oracle's answer here."""
import numpy as np
import pytest

from bench import parity_relerr, parity_relerr_elementwise
from conftest import LIMITS

pytestmark = pytest.mark.gpu

REL = 1e-9
NTHREADS = 16
EXACT = (3, 4, 5, 7, 9, 10, 11)       # fp64 default order: the reference's operation order, the oracle's bits
FUSED = (1, 2, 6, 8)                  # fused forms, within 1e-9 (critical rays re-traced in reference order)
DX, DTH = 1e-3, 1e-4


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = __import__("ctypes").c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


@pytest.fixture(scope="module")
def gpu_fields(rb):
    cache = {}

    def get(scen, dtype=0):
        key = ("vert_heterogeneous" if scen == "anisotropy" else scen, dtype)
        if key not in cache:
            cache[key] = rb.Field.build(key[0], LIMITS[key[0]], rb.DELTA, dtype)
        return cache[key]
    yield get
    for f in cache.values():
        f.close()


def relerr(a, b):
    return max(parity_relerr(a, b), parity_relerr_elementwise(a, b))


def perturbed_states(OF, m, gam, step, box, x0, y0, th, k):
    """The oracle's rays stopped at row k (max_size = k + 1), those still under way, perturbed: (state9, hist4 or None)."""
    from oracle import rt_oracle as O
    r = O.trazar(OF, m, gam, step, k + 1, box, x0, y0, th, record_stride=1 if m == 7 else 0, rec_rows=k + 1,
                 nthreads=NTHREADS)
    live = r["d_ray"][2] == k
    fin, d = r["final"][:, live], r["d_ray"][:, live]
    st9 = np.concatenate([fin[:6], d[1:2], d[0:1], fin[8:9]])          # d_ray holds dist_real, dist_sim
    st9[0] += DX
    st9[2] += DTH
    st9[3:6] = np.stack(OF.n_gradient(st9[0], st9[1]))
    hist4 = None
    if m == 7:
        s = r["s_ray"][:, :, live]
        hist4 = np.concatenate([s[k - 2, :2], s[k - 1, :2]])
        hist4[[0, 2]] += DX
    return st9, hist4


def device_run(rb, F, m, gam, step, ms, box, st9, hist4, istep, kw, mode="auto", stepped=0, th0=None, x0=-2.0, **bkw):
    """A batch launched from unrelated conditions, given the states, run to its end: (rows, final, d_ray, stats, row 0)."""
    R = st9.shape[1]
    th0 = np.full(R, np.pi / 4) if th0 is None else th0
    b = rb.Batch(F, m, step, ms, box, gam, th0, x0, -2.0, launch_mode=mode, **kw, **bkw)
    row0 = b.rows(0, 1) if kw.get("record_stride", 1) else None
    b.set_state(st9, hist4, np.broadcast_to(np.asarray(istep, dtype=np.int32), (R,)))
    if stepped:
        while True:
            b.step(stepped)
            if b.stats()["live_rays"] == 0:
                break
    else:
        b.run()
    out = (b.rows() if kw.get("record_stride", 1) else None, b.final(), b.d_ray(), b.stats(), row0)
    b.close()
    return out


def check_rows(s, row0, istep, stride):
    """Rows at or before each ray's istep are what they were before the run (row 0 of the launch conditions, zeros); the
    rows after it are the oracle's continuation (whose rows at or before istep are zeros)."""
    first = np.asarray(istep) // stride + 1
    for f in np.unique(first):
        sel = first == f
        assert np.array_equal(s[0][:, sel], row0[0][:, sel])
        assert not s[1:f][:, :, sel].any()


def fan(scen, R):
    """The launch fan the states are taken from, and the run's step / max_size."""
    if scen == "fisheye":
        return 1.0, 0.0, np.linspace(np.pi / 4, 3 * np.pi / 4, R), 2 * np.pi / 303, 10 * 304
    from raytracing_amd import rt_bench as rb
    return -2.0, -2.0, np.linspace(0.1, np.pi / 2, R), rb.DELTA_S, int(np.ceil(80 / rb.DELTA_S) + 1)


CASES = [(s, m, 1) for s in ("fisheye", "vert_heterogeneous", "interface") for m in range(1, 10)] + \
        [("anisotropy", 10, 3), ("anisotropy", 11, 3)]


@pytest.mark.parametrize("scen,m,gam", CASES)
def test_set_state_vs_oracle_continuation(scen, m, gam, rb, gpu_fields, oracle_fields):
    """Every method on every scenario, the rays of a 256-ray fan still under way at row 300, perturbed, given to a batch launched elsewhere: the
    reference-order methods give the oracle's bits, op1/2/6/8 are within 1e-9 on every ray with equal step counts (and with
    reference_order the oracle's bits); rows at or before istep are untouched."""
    from oracle import rt_oracle as O
    OF = oracle_fields(scen)
    box = LIMITS[scen]
    x0, y0, th, step, ms = fan(scen, 256)
    k, stride = 300, 7
    st9, hist4 = perturbed_states(OF, m, gam, step, box, x0, y0, th, k)
    R = st9.shape[1]
    assert R >= 100
    rows = (ms + stride - 1) // stride
    kw = dict(record_stride=stride, rec_rows=rows)
    o = O.trazar_from_state(OF, m, gam, step, ms, box, st9, hist4, k, nthreads=NTHREADS, **kw)
    orders = [False, True] if m in FUSED else [False]
    for ro in orders:
        s, fin, d, st, row0 = device_run(rb, gpu_fields(scen), m, gam, step, ms, box, st9, hist4, k, kw, reference_order=ro)
        check_rows(s, row0, np.full(R, k), stride)
        first = k // stride + 1
        assert np.array_equal(d[2], o["d_ray"][2])
        if m in EXACT or ro:
            assert np.array_equal(s[first:], o["s_ray"][first:]) and np.array_equal(fin, o["final"])
            assert np.array_equal(d, o["d_ray"])
        else:
            assert relerr(s[first:], o["s_ray"][first:]) < REL
            assert relerr(fin, o["final"]) < REL and relerr(d[:2], o["d_ray"][:2]) < REL
        assert st["retrace_overflow"] == 0


# ------------------------------------------------------------------ critical rays re-traced from the state that was set
_WINDOWS = {6: 487296, 8: 487168, 1: 483328, 2: 483328}       # test_critical_rays_of_the_1m_interface_fan
_CRIT_K = 800                                                 # before the rays hover (they do at row 1 250)
_crit_cache = {}


def critical_window(m, rb, OF):
    """The 1 024-ray interface window around method m's split, stopped at row 800 and perturbed, and the oracle's continuation."""
    from oracle import rt_oracle as O
    if m not in _crit_cache:
        th = np.linspace(2 * np.pi / 60, np.pi / 2, 1 << 20)[_WINDOWS[m]:_WINDOWS[m] + 1024]
        lim = LIMITS["interface"]
        ms = int(np.ceil(80 / rb.DELTA_S) + 1)
        st9, _ = perturbed_states(OF, m, 1, rb.DELTA_S, lim, -2.0, -2.0, th, _CRIT_K)
        kw = dict(record_stride=16, rec_rows=600)
        o = O.trazar_from_state(OF, m, 1, rb.DELTA_S, ms, lim, st9, None, _CRIT_K, nthreads=NTHREADS, **kw)
        _crit_cache[m] = (st9, o, ms, kw)
    return _crit_cache[m]


@pytest.mark.parametrize("m,mode", [(6, "plain"), (8, "plain"), (1, "plain"), (2, "plain"), (6, "sliced"), (6, "refill"),
                                    (6, "steps"), (6, "sorted")])
def test_critical_rays_retraced_from_the_state_that_was_set(m, mode, rb, gpu_fields, oracle_fields):
    """A default batch (retrace on) given states near the interface's critical angle: some rays hover and are re-traced in
    reference order -- from the state that was set: a re-trace from the launch conditions would be nowhere near -- and every
    ray is within 1e-10 of the oracle (rows, per quantity) with equal step counts, in every schedule and with sort_rays
    (k_set_state maps caller order to slot order).  (A re-traced ray goes back to the fused form once it has left the wall,
    so its end is the fused form's, not the oracle's bits.)"""
    st9, o, ms, kw = critical_window(m, rb, oracle_fields("interface"))
    R = st9.shape[1]
    lim = LIMITS["interface"]
    extra = {}
    if mode == "sorted":
        rng = np.random.default_rng(5)
        extra = dict(sort_rays=True, th0=rng.permutation(np.linspace(0.1, 1.4, R)), x0=np.where(rng.random(R) < 0.3, -1.0, -2.0))
    s, fin, d, st, row0 = device_run(rb, gpu_fields("interface"), m, 1, rb.DELTA_S, ms, lim, st9, None, _CRIT_K, kw,
                                     mode={"steps": "plain", "sorted": "plain"}.get(mode, mode),
                                     stepped=300 if mode == "steps" else 0, **extra)
    print(f"op{m} {mode}: {st['retraced']} of {R} rays re-traced; {relerr(fin, o['final']):.1e} from the oracle (final state)")
    assert st["retraced"] > 0 and st["retrace_overflow"] == 0
    check_rows(s, row0, np.full(R, _CRIT_K), 16)
    first = _CRIT_K // 16 + 1
    assert np.array_equal(d[2], o["d_ray"][2])
    a, w = s[first:], o["s_ray"][first:]
    dev = np.array([np.abs(a[:, q] - w[:, q]).max(axis=(0, 1)) / np.abs(w[:, q]).max() for q in ([0, 1], [2, 3], [4], [5])]).max(axis=0)
    assert (dev > REL).sum() == 0 and dev.max() < 1e-10, f"{int((dev > REL).sum())} rays beyond 1e-9, largest {dev.max():.1e}"
    assert relerr(a, w) < REL
    assert relerr(fin, o["final"]) < REL and relerr(d[:2], o["d_ray"][:2]) < REL


def test_set_state_discards_a_pending_hand_over(rb, gpu_fields, oracle_fields):
    """rtmi_step hands critical rays over and nothing reads them; set_state then replaces every ray's state.  The next run must
    not see the old rays' re-trace: the result is bit for bit that of a fresh batch given the same states."""
    from oracle import rt_oracle as O
    F, OF = gpu_fields("interface"), oracle_fields("interface")
    lim = LIMITS["interface"]
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    th_win = np.linspace(2 * np.pi / 60, np.pi / 2, 1 << 20)[_WINDOWS[6]:_WINDOWS[6] + 1024]
    kw = dict(record_stride=16, rec_rows=600)
    # how many steps until the window has handed rays over (read on a probe batch: a read drains its queue)
    probe = rb.Batch(F, 6, rb.DELTA_S, ms, lim, 1, th_win, -2.0, -2.0, **kw)
    n = 0
    while probe.stats()["retraced"] == 0:
        assert n < 6000, "the window never handed a ray over"
        probe.step(250)
        n += 250
    probe.close()
    # states far from the critical angle: nothing of theirs is handed over
    st9, _ = perturbed_states(OF, 6, 1, rb.DELTA_S, lim, -2.0, -2.0, np.linspace(0.2, 0.6, 1024), 300)
    R = st9.shape[1]
    st9 = np.pad(st9, ((0, 0), (0, 1024 - R)), mode="edge")
    istep = np.full(1024, 300, np.int32)
    a = rb.Batch(F, 6, rb.DELTA_S, ms, lim, 1, th_win, -2.0, -2.0, **kw)
    a.step(n)                                                   # rays handed over, unread
    a.set_state(st9, None, istep)
    a.run()
    got = (a.rows(), a.final(), a.d_ray())
    a.close()
    b = rb.Batch(F, 6, rb.DELTA_S, ms, lim, 1, th_win, -2.0, -2.0, **kw)
    b.set_state(st9, None, istep)
    b.run()
    ref = (b.rows(), b.final(), b.d_ray())
    b.close()
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    # the rows this run wrote (set_state keeps the rows at or before istep, and a's stepping wrote some of those)
    r = np.arange(600)[:, None] * 16
    ran = (r > istep[None, :]) & (r <= ref[2][2][None, :])
    assert ran.any(axis=0).all()
    assert np.array_equal(np.where(ran[:, None, :], got[0], 0), np.where(ran[:, None, :], ref[0], 0))
    o = O.trazar_from_state(OF, 6, 1, rb.DELTA_S, ms, lim, st9, None, istep, nthreads=NTHREADS, **kw)
    assert np.array_equal(got[2][2], o["d_ray"][2]) and relerr(got[1], o["final"]) < REL


@pytest.mark.parametrize("m", [6, 3, 7, 2])
def test_set_state_edges(m, rb, gpu_fields, oracle_fields):
    """istep = max_size - 2: exactly one step; istep = max_size - 1: none, the final state is the one set; a state outside
    the box: exactly one step (the box test follows the step, :878); op7 with a caller-given history at istep 2 and 900."""
    from oracle import rt_oracle as O
    scen = "vert_heterogeneous"
    OF, box = oracle_fields(scen), LIMITS[scen]
    x0, y0, th, step, ms = fan(scen, 64)
    parts = []
    for k in (2, 900):
        st9, hist4 = perturbed_states(OF, m, 1, step, box, x0, y0, th, k)
        parts.append((st9[:, :32], hist4[:, :32] if hist4 is not None else None, np.full(32, k)))
    st9 = np.concatenate([p[0] for p in parts], axis=1)
    hist4 = np.concatenate([p[1] for p in parts], axis=1) if m == 7 else None
    istep = np.concatenate([p[2] for p in parts]).astype(np.int32)
    R = st9.shape[1]
    istep[40:44] = ms - 2
    istep[44:48] = ms - 1
    st9[0, 48:52] = box[1] + 0.05                               # outside the box
    st9[1, 52:56] = box[2] - 0.05
    st9[3:6, 48:56] = np.stack(OF.n_gradient(st9[0, 48:56], st9[1, 48:56]))
    kw = dict(record_stride=1, rec_rows=ms)
    o = O.trazar_from_state(OF, m, 1, step, ms, box, st9, hist4, istep, nthreads=NTHREADS, **kw)
    assert np.array_equal(o["d_ray"][2, 40:48], np.repeat([ms - 1], 8))
    assert np.array_equal(o["d_ray"][2, 48:56], istep[48:56] + 1)
    s, fin, d, st, row0 = device_run(rb, gpu_fields(scen), m, 1, step, ms, box, st9, hist4, istep, kw)
    assert np.array_equal(d[2], o["d_ray"][2])
    assert np.array_equal(fin[:6, 44:48], st9[:6, 44:48]) and np.array_equal(fin[8, 44:48], st9[8, 44:48])
    assert np.array_equal(d[0, 44:48], st9[7, 44:48]) and np.array_equal(d[1, 44:48], st9[6, 44:48])
    check_rows(s, row0, istep, 1)
    after = np.arange(ms)[:, None, None] > istep[None, None, :]          # the oracle's rows at or before istep are zeros
    if m in EXACT:
        assert np.array_equal(np.where(after, s, 0), o["s_ray"])
        assert np.array_equal(fin, o["final"]) and np.array_equal(d, o["d_ray"])
    else:
        mask = after
        assert relerr(np.where(mask, s, 0), np.where(mask, o["s_ray"], 0)) < REL
        assert relerr(fin, o["final"]) < REL and relerr(d[:2], o["d_ray"][:2]) < REL


def test_fp32_set_state_tracks_the_fp64_oracle(rb, gpu_fields, oracle_fields):
    """fp32 batches given the states: the fp64 oracle's continuation within test_fp32_path_tracks_fp64's tolerances.  (Not op7:
    its fp32 form differentiates fp32 positions, and its step counts wander by tens from the fp64 ones from any start.)"""
    from oracle import rt_oracle as O
    scen = "vert_heterogeneous"
    OF, box = oracle_fields(scen), LIMITS[scen]
    x0, y0, th, step, ms = fan(scen, 512)
    for m in (6, 2, 8):
        st9, hist4 = perturbed_states(OF, m, 1, step, box, x0, y0, th, 300)
        R = st9.shape[1]
        o = O.trazar_from_state(OF, m, 1, step, ms, box, st9, hist4, 300, record_stride=0, nthreads=NTHREADS)
        _, fin, d, _, _ = device_run(rb, gpu_fields(scen, 1), m, 1, step, ms, box, st9, hist4, 300, dict(record_stride=0))
        assert np.max(np.abs(d[2] - o["d_ray"][2])) <= 1
        same = d[2] == o["d_ray"][2]
        err = np.abs(fin[:2] - o["final"][:2])[:, same].max()
        print(f"op{m} fp32 from set states: same step count on {same.sum()}/{R} rays, end-point max abs error {err:.3e}")
        assert same.mean() > 0.98 and err < 2e-5


@pytest.mark.parametrize("m", [6, 8, 1, 2])
@pytest.mark.parametrize("mult", [1, 50])
def test_step_token_on_grazing_interface_states(m, mult, rb, gpu_fields, oracle_fields):
    """op<m>(...) -- StepMethod.__call__, the reference's call surface -- on the interface field from states grazing the
    interface inside its steep band (|grad n| up to 11, headings within 1.2 degrees of it), at DELTA_S and at 50 DELTA_S:
    one step, within 1e-12 of the oracle's single step."""
    from oracle import rt_oracle as O
    F, OF = gpu_fields("interface"), oracle_fields("interface")
    y = np.linspace(-0.012, 0.012, 9)
    x = 2.0 + np.arange(len(y)) * 0.7
    th = np.array([0.02, -0.015, 0.01, -0.005, 0.0, 0.005, -0.01, 0.015, -0.02])
    n, gx, gy = OF.n_gradient(x, y)
    assert np.abs(np.hypot(gx, gy)).max() > 10.0                 # inside the steep band
    z, grd = rb.FieldSpline(F, "n"), (rb.FieldSpline(F, "dy"), rb.FieldSpline(F, "dx"))
    step = mult * rb.DELTA_S
    full = np.stack([x, y, th, n, gx, gy, np.ones(len(y))], axis=1)
    ref = O.single_step(OF, m, 1, step, full)
    for q in range(len(y)):
        u = np.array((np.cos(th[q]), np.sin(th[q])))
        fp, fa, fn, fg = getattr(rb, f"op{m}")(th[q], n[q], np.array((gx[q], gy[q])), u, np.array((x[q], y[q])), 1.0, grd, z, step)
        got = np.array([fp[0], fp[1], fa, fn, fg[0], fg[1]])
        err = np.abs(got - ref[q]) / np.maximum(np.abs(ref[q]), 1e-3)
        err[2] = abs(got[2] - ref[q, 2])
        assert err.max() < 1e-12, (q, err)
