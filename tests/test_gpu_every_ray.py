"""GPU: every ray of the 1 048 576-ray fans, not a sample.  A reference-order batch (rtmi_params.reference_order = 1: op1/2/6/8
give the oracle's bits) is the reference ON THE DEVICE, anchored to the oracle on every 1 024th ray; a default batch of the same
fan is then compared with it ray by ray (tests/every_ray.py: bench.parity_relerr's per-quantity measure and the element-wise
one, the larger, NaN an offender), the recorded rows in chunks of rays without leaving the device.  What the fused forms and the
hand-over of critical rays (the hover sum, rt_device.h) must give is then checked on all R rays: equal step counts and 0 rays
beyond 1e-9 -- where tests/test_gpu_parity.py looks at every 512th ray and at windows around the interface fan's split."""
import numpy as np
import pytest

from bench import SCEN
from conftest import LIMITS
from every_ray import Compared, fingerprint

pytestmark = pytest.mark.gpu

REL = 1e-9
R = 1 << 20
ANCHOR = 1024
R_CFG4 = 1 << 23                  # test_cfg4_fp32_full_8m_rays's fan
FAST_FIELD = 1e-10                # rtmi.h: RTMI_ORDER_FAST_FIELD's distance from the reference away from sharp interfaces
N0 = 0.07142864686293911          # vert_heterogeneous: n at the launch point; p_x = N0 cos(theta) is conserved


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench
    import torch
    assert torch.cuda.is_available(), "no HIP device"
    return rt_bench


@pytest.fixture(scope="module")
def gpu_fields(rb):
    cache = {}

    def get(scen, dtype=0):
        if (scen, dtype) not in cache:
            cache[scen, dtype] = rb.Field.build(scen, LIMITS[scen], rb.DELTA, dtype)
        return cache[scen, dtype]
    yield get
    for f in cache.values():
        f.close()


def plan(rb, scen):
    """(DELTA_S, max_size, record_stride, rec_rows) of the 1 M-ray tests and tools/parity_sweep_1m.py (fisheye: rec_rows 0, the
    library sizes the record: 190 rows)."""
    if scen == "fisheye":
        return 2 * np.pi / 303, rb.N * 304, 16, 0
    return rb.DELTA_S, int(np.ceil(80 / rb.DELTA_S) + 1), 16, (600 if scen == "interface" else 192)


def tilted_wall(rb, O, tilt_deg):
    """The interface scenario's sigmoid wall tilted against the grid, as samples on both sides (test_critical_rays_of_a_tilted_wall)."""
    x, y = O.Field("interface", LIMITS["interface"], rb.DELTA).arrays()[:2]
    X, Y = np.meshgrid(x, y)
    a = np.radians(tilt_deg)
    d = -np.sin(a) * (X + 2.0) + np.cos(a) * Y
    Z = np.sqrt(2.0) - (np.sqrt(2.0) - 1.0) / (1.0 + np.exp(-np.clip(d / 0.005, -700, 700)))
    return rb.Field.from_samples(x, y, Z, rb.DELTA), O.Field.from_samples(x, y, Z, rb.DELTA)


class Batches:
    """Closes every batch it made (30 GB each on the interface fan) and returns the cache's chunk temporaries to the device
    before the next test creates its own."""

    def __init__(self, rb):
        self.rb, self.open = rb, []

    def make(self, *args, **kw):
        import torch
        b = self.rb.Batch(*args, **kw)
        self.open.append(b)
        b.run()
        torch.cuda.synchronize()
        return b

    def close(self, b):
        import torch
        torch.cuda.synchronize()
        b.close()
        self.open.remove(b)
        torch.cuda.empty_cache()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in list(self.open):
            self.close(b)


def anchor(o, b, sub):
    """The batch's d_ray, final state and recorded rows of the rays `sub` equal the oracle's bits."""
    assert np.array_equal(b.d_ray()[:, sub], o["d_ray"])
    assert np.array_equal(b.final()[:, sub], o["final"])
    if "s_ray" in b.device_tensors():
        got = b.device_tensors()["s_ray"][:, :, sub].cpu().numpy()
        assert got.shape == o["s_ray"].shape and np.array_equal(got, o["s_ray"])


def compare(b, ref, th):
    """Step counts (mismatching rays) and per-ray comparisons of the final state, d_ray[:2] and the recorded rows."""
    d, dr = b.d_ray(), ref.d_ray()
    steps = np.nonzero(d[2] != dr[2])[0]
    parts = {"final": Compared(b.final(), ref.final(), th), "d_ray": Compared(d[:2], dr[:2], th)}
    t, tr = b.device_tensors(), ref.device_tensors()
    if "s_ray" in tr:
        parts["rows"] = Compared(t["s_ray"], tr["s_ray"], th)
    return steps, parts


def summary(parts, tol):
    return ", ".join(f"{k} max {c.max:.2e} ({len(c.beyond(tol))} beyond {tol:g}; worst {c.report(1)})" for k, c in parts.items())


def union_beyond(parts, tol):
    out = np.zeros(0, np.int64)
    for c in parts.values():
        out = np.union1d(out, c.beyond(tol))
    return out


CONFIGS = [(s, m, None) for s in ("vert_heterogeneous", "fisheye", "interface") for m in (1, 2, 6, 8)] + \
          [("interface", 6, 3.0), ("interface", 6, 11.0), ("interface", 1, 11.0)]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("scen, method, tilt", CONFIGS,
                         ids=[f"{s}-op{m}" if t is None else f"tilted{t:g}-op{m}" for s, m, t in CONFIGS])
def test_every_ray_of_the_1m_fan(scen, method, tilt, rb, gpu_fields, oracle_fields):
    """One fan, 1 048 576 rays, every 16th row recorded: (1) the reference-order batch is the oracle's bits on every 1 024th ray;
    (2) a default batch (launch_mode auto, the re-trace on) has the reference-order batch's step count on EVERY ray and 0 rays
    beyond 1e-9 in the final state, d_ray and every recorded row -- on vert_heterogeneous and fisheye (no sharp transition,
    nothing ill-conditioned) also below 1e-11; (3) critical rays are re-traced where there is a wall and only there, with room in
    the queue; (4) the re-run -- the AUTO exploration's other schedule, the critical bundles dispatched first -- gives every ray's
    bits again; (5) on the interface fan the same comparison finds offenders when the re-trace is off: it is not blind."""
    import torch
    from oracle import rt_oracle as O
    sc = SCEN[scen]
    th = np.linspace(*sc["theta"], R)
    x0, y0 = sc["start"]
    lim = LIMITS[scen]
    step, ms, stride, rows = plan(rb, scen)
    if tilt is None:
        F, OF = gpu_fields(scen), oracle_fields(scen)
    else:
        F, OF = tilted_wall(rb, O, tilt)
    name = f"{scen if tilt is None else f'wall tilted {tilt:g} deg'} op{method}"
    kw = dict(record_stride=stride, rec_rows=rows, keep_n_ray=False)
    args = (F, method, step, ms, lim, 1, th, x0, y0)
    wall = scen == "interface"
    try:
        with Batches(rb) as B:
            ref = B.make(*args, reference_order=True, **kw)
            st_ref = ref.stats()
            assert st_ref["live_rays"] == 0 and st_ref["ray_steps"] == int(ref.d_ray()[2].sum())
            # (1) the anchor: the reference-order batch of THIS size (field path and schedule depend on R) is the oracle's bits
            sub = slice(0, R, ANCHOR)
            o = O.trazar(OF, method, 1, step, ms, lim, x0, y0, th[sub], record_stride=stride, rec_rows=rows or None, nthreads=16)
            anchor(o, ref, sub)

            # (2) every ray of a default batch
            b = B.make(*args, **kw)
            st = b.stats()
            steps, parts = compare(b, ref, th)
            print(f"\n{name}: {R} rays, retraced {st['retraced']} (overflow {st['retrace_overflow']}), schedule {st['launch_mode_used']}; "
                  f"{len(steps)} step counts differ; {summary(parts, REL)}")
            assert len(steps) == 0, f"{name}: step counts differ on {len(steps)} rays, e.g. " + \
                "; ".join(f"ray {i} (theta {th[i]:.15g}) {int(b.d_ray()[2][i])} vs {int(ref.d_ray()[2][i])}" for i in steps[:5])
            for k, c in parts.items():
                bad = c.beyond(REL)
                assert len(bad) == 0, f"{name}: {len(bad)} rays of the {k} beyond 1e-9, the worst: {c.report(5)}"
            if not wall:
                for k, c in parts.items():
                    assert c.max < 1e-11, f"{name}: {k} {c.report(3)}"

            # (3) the hand-over's bookkeeping
            assert st["live_rays"] == 0 and st["ray_steps"] == int(b.d_ray()[2].sum()) == st_ref["ray_steps"]
            if wall:
                assert 0 < st["retraced"] and st["retrace_overflow"] == 0
            else:
                assert st["retraced"] == 0

            # (4) the re-run: every ray's bits again
            d1, f1 = b.d_ray(), b.final()
            fp1 = fingerprint(b.device_tensors()["s_ray"])
            b.reset()
            b.run()
            torch.cuda.synchronize()
            st2 = b.stats()
            print(f"{name}: re-run schedule {st2['launch_mode_used']}, dispatch_first {st2['dispatch_first']}, retraced {st2['retraced']}")
            assert st2["ray_steps"] == st["ray_steps"] and st2["retraced"] == st["retraced"] and st2["retrace_overflow"] == 0
            assert np.array_equal(b.d_ray(), d1) and np.array_equal(b.final(), f1)
            moved = torch.nonzero((fingerprint(b.device_tensors()["s_ray"]) != fp1).any(dim=0)).flatten().cpu().numpy()
            assert len(moved) == 0, f"{name}: the re-run's rows differ on {len(moved)} rays, e.g. {moved[:5]}"
            del fp1, parts
            B.close(b)

            # (5) the comparator sees the fused forms' offenders when nothing hands them over
            if wall and tilt is None:
                b0 = B.make(*args, retrace=False, **kw)
                st0 = b0.stats()
                steps0, parts0 = compare(b0, ref, th)
                bad0 = np.union1d(steps0, union_beyond(parts0, REL))
                print(f"{name} with the re-trace off: {len(bad0)} rays beyond 1e-9 or with another step count ({summary(parts0, REL)})")
                assert st0["retraced"] == 0 and len(bad0) >= 1
                del parts0
    finally:
        if tilt is not None:
            F.close()
        torch.cuda.empty_cache()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("scen", ["vert_heterogeneous", "fisheye"])
def test_op7_fast_field_on_every_ray(scen, rb, gpu_fields, oracle_fields):
    """op7 with reference_order="fast_field" (its reference-order step on the fused field lookup) against the default op7 batch
    (reference order throughout: the oracle's bits, anchored on every 1 024th ray), 1 048 576 rays: equal step counts and every
    ray within rtmi.h's 1e-10 -- whose only exception, rays grazing a sharp interface, these fields do not have.  Measured on
    every ray: 9.5e-11 (vert_heterogeneous, ray 398 754) and 3.5e-11 (fisheye).  The 4 096-ray fans of the parity sweep had
    shown 4e-11 and the header said 8e-11: the error is a random walk of the lookup's last-bit differences through op7's
    differenced positions over a ray's ~2 800 steps (no one step adds more than 5e-14), and a million rays reach further into
    its tail than four thousand."""
    import torch
    from oracle import rt_oracle as O
    sc = SCEN[scen]
    th = np.linspace(*sc["theta"], R)
    x0, y0 = sc["start"]
    lim = LIMITS[scen]
    step, ms, stride, rows = plan(rb, scen)
    F = gpu_fields(scen)
    kw = dict(record_stride=stride, rec_rows=rows, keep_n_ray=False)
    args = (F, 7, step, ms, lim, 1, th, x0, y0)
    try:
        with Batches(rb) as B:
            ref = B.make(*args, **kw)
            sub = slice(0, R, ANCHOR)
            o = O.trazar(oracle_fields(scen), 7, 1, step, ms, lim, x0, y0, th[sub], record_stride=stride, rec_rows=rows or None, nthreads=16)
            anchor(o, ref, sub)
            b = B.make(*args, reference_order="fast_field", **kw)
            steps, parts = compare(b, ref, th)
            print(f"\n{scen} op7 fast_field: {len(steps)} step counts differ; {summary(parts, FAST_FIELD)}")
            assert len(steps) == 0, f"step counts differ on rays {steps[:5]}"
            for k, c in parts.items():
                assert len(c.beyond(FAST_FIELD)) == 0, f"{scen} op7 fast_field, {k}: {len(c.beyond(FAST_FIELD))} rays beyond 1e-10: {c.report(5)}"
            del parts
    finally:
        torch.cuda.empty_cache()


@pytest.mark.timeout(900)
def test_cfg4_fp32_every_ray_of_8m(rb, gpu_fields, oracle_fields):
    """test_cfg4_fp32_full_8m_rays's bounds on ALL 8 388 608 rays: the fp32 op6 batch against an fp64 reference-order batch of the
    same fan (the oracle's bits, anchored on every 8 192nd ray), compared on the device -- x, y, T and both arclengths are fp64
    accumulators in both precisions.  Step counts never more than one row apart and equal on >= 99 % of the rays; on those, end
    points within 2e-5, traveltime within 2e-5 of its scale, arclengths within 1e-5 of theirs; p_x conserved over the fan."""
    import torch
    from oracle import rt_oracle as O
    R8 = R_CFG4
    th = np.linspace(0, np.pi / 2, R8)
    lim = LIMITS["vert_heterogeneous"]
    step, ms = rb.DELTA_S, int(np.ceil(80 / rb.DELTA_S) + 1)
    try:
        with Batches(rb) as B:
            b64 = B.make(gpu_fields("vert_heterogeneous"), 6, step, ms, lim, 1, th, -2.0, -2.0, record_stride=0, reference_order=True)
            sub = slice(0, R8, R8 // ANCHOR)
            o = O.trazar(oracle_fields("vert_heterogeneous"), 6, 1, step, ms, lim, -2.0, -2.0, th[sub], record_stride=0, nthreads=16)
            anchor(o, b64, sub)
            b32 = B.make(gpu_fields("vert_heterogeneous", 1), 6, step, ms, lim, 1, th, -2.0, -2.0, record_stride=0)
            st = b32.stats()
            assert st["live_rays"] == 0
            t32, t64 = b32.device_tensors(), b64.device_tensors()
            dstep = (t32["istep"].long() - t64["istep"].long()).abs()
            assert st["ray_steps"] == int(t32["istep"].long().sum())
            same = dstep == 0
            e_xy = torch.maximum((t32["x"] - t64["x"]).abs(), (t32["y"] - t64["y"]).abs())
            e_T = (t32["T"] - t64["T"]).abs() / t64["T"].abs().max()
            s64 = torch.stack([t64["dist_real"], t64["dist_sim"]])
            e_s = (torch.stack([t32["dist_real"], t32["dist_sim"]]) - s64).abs().amax(dim=0) / s64.abs().max()
            errs = {"end point": (e_xy, 2e-5), "traveltime": (e_T, 2e-5), "arclength": (e_s, 1e-5)}
            worst_of = {k: float(torch.where(same, e, torch.zeros_like(e)).nan_to_num(nan=float("inf")).max()) for k, (e, _) in errs.items()}
            print(f"\ncfg4 fp32 vs fp64 reference order on all {R8} rays: step count equal on {float(same.double().mean()):.4%} "
                  f"(largest difference {int(dstep.max())} row); on those: " + ", ".join(f"{k} {v:.2e}" for k, v in worst_of.items()))
            assert int(dstep.max()) <= 1 and float(same.double().mean()) >= 0.99
            for k, (e, tol) in errs.items():
                bad = torch.nonzero(same & ~(e <= tol)).flatten().cpu().numpy()
                assert len(bad) == 0, f"cfg4 {k}: {len(bad)} rays beyond {tol:g}: " + \
                    "; ".join(f"ray {i} (theta {th[i]:.15g}) {float(e[i]):.3e}" for i in bad[:5])
            f32 = b32.final()
            assert np.max(np.abs(f32[6] - N0 * np.cos(th))) / N0 < 6e-4
            del t32, t64, e_xy, e_T, e_s, s64, errs, same, dstep
    finally:
        torch.cuda.empty_cache()
