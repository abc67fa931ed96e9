"""Host API for the MI355X ray propagation path -- the selection surface of neyuru/RayTracing's
RT_bench.py (scenarios, step methods op1..op11, DELTA_S stepping, trazar) over librtmi.so.

Names, argument order and return shapes follow the reference so a caller of
`genZ` / `interpolacion` / `n_gradient` / `trazar` / `search_delta` can switch imports; all numerics
run in HIP kernels on the GPU (see include/rtmi.h).  Reference lines are RT_bench.py file:line.
There is no CPU path here: without a HIP device every compute call raises.
"""
import ctypes as C
import time

import numpy as np

from . import _lib
from ._lib import Params, Stats, DeviceView, check, dptr, lib, LAUNCH_MODES, LAUNCH_NAMES, LAUNCH_AUTO, LAUNCH_REFILL, LAUNCH_SLICED, LAUNCH_PLAIN

# re-runs of one batch (reset + run) RTMI_LAUNCH_AUTO spends timing its two schedules before it keeps one (rtmi.h: RTMI_AUTO_SAMPLES each)
AUTO_EXPLORE_RUNS = 2 * _lib.AUTO_SAMPLES

# --------------------------------------------------------------------------- constants (:59-97)
THCK_PARAM = 0.005                                   # :59
SIGMA = 0.05293304824724534                          # :60-61 (value of -2*THCK*log((A-1)/(sqrt2-A)) under numpy)
DELTA_G = np.pi / 2                                  # :64
GOLD_RATIO = (np.sqrt(5) - 1) / 2                    # :65
GOLD_TOL = 1.4901161193847656e-08                    # :66 sqrt(eps)
MAX_DEVIATION = 0.2                                  # :69
DELTA = SIGMA / 3                                    # :77
DELTA_S_DIVISOR = 20                                 # :79
DELTA_S = SIGMA / DELTA_S_DIVISOR                    # :81
N = 10                                               # :82
DELTA_S_DIVISOR_FISHEYE = 90                         # :84
DELTA_STEP = 0.01                                    # :89
DELTA_S_DIVISOR_UPPER_LIMIT = 3                      # :90
DELTA_S_DIVISOR_LOWER_LIMIT = 1 + DELTA_STEP         # :91
DELTA_STEP_FISHEYE = 1                               # :92
DELTA_S_DIVISOR_FISHEYE_UPPER_LIMIT = 303            # :93
DELTA_S_DIVISOR_FISHEYE_LOWER_LIMIT = 4              # :94
DELTA_STEP_VERT = 0.005                              # :95
DELTA_S_DIVISOR_VERT_UPPER_LIMIT = 2                 # :96
DELTA_S_DIVISOR_VERT_LOWER_LIMIT = 1 / 40            # :97

F64, F32 = 0, 1
ORDERS = {"default": 0, "reference": 1, "fused": 2, "fast_field": 3}          # rtmi_order (rtmi_params.reference_order)


# --------------------------------------------------------------------------- scenarios (:106-119)
class Scenario:
    """A scenario token.  genZ() samples it on the device; calling it evaluates the same formula with
    numpy for callers that only want to look at n(x, y) (plots, docs) -- it is not on the trace path."""

    def __init__(self, name, code, fn):
        self.__name__ = name
        self.code = code
        self._fn = fn

    def __call__(self, a, b):
        return self._fn(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))

    def __repr__(self):
        return f"<scenario {self.__name__}>"


interface = Scenario("interface", 1, lambda a, b: np.sqrt(2) - (np.sqrt(2) - 1) / (1 + np.exp(-b / THCK_PARAM)))
fisheye = Scenario("fisheye", 2, lambda a, b: 1 / (1 + np.power(a, 2) + np.power(b, 2)))
vert_heterogeneous = Scenario("vert_heterogeneous", 3, lambda a, b: 1 / (18 + 2 * b))
SCENARIOS = {"interface": interface, "fisheye": fisheye, "vert_heterogeneous": vert_heterogeneous,
             "anisotropy": vert_heterogeneous}          # scenario 4 reuses the field of 3 (:1579)
USER_CHOICE = {"interface": "1", "fisheye": "2", "vert_heterogeneous": "3", "anisotropy": "4"}

# module globals the reference's __main__ sets (:1567-1584); genZ reads `f` like the reference does (:432)
f = None
gamma = 1


def anisotropy(theta, gamma):  # :118-119 (host helper; the device evaluates its own copy)
    return np.sqrt((gamma * np.sin(theta)) ** 2 + np.cos(theta) ** 2)


def constants(user_choice):
    """Scenario presets, same 13-tuple as RT_bench.py:247-295."""
    if user_choice == "1":
        g, ray_count = 1, 42
        theta_v = np.linspace(2 * (np.pi / 60), np.pi / 2, ray_count + 1)   # Q9: one unused sample
        pos_x = np.ones(ray_count) * -2
        s = 80
        lim = (-2, 20, -2, 4)
        flags = (1, 0, 0, 0)
    elif user_choice == "2":
        g, ray_count = 1, 1
        theta_v = np.linspace(np.pi / 2, np.pi / 2, 1)
        pos_x = np.array((1, 0))
        s = N * (2 * np.pi)
        lim = (-1.5, 1.5, -1.5, 1.5)
        flags = (0, 1, 0, 0)
    elif user_choice in ("3", "4"):
        g = 1 if user_choice == "3" else 3
        ray_count = 31
        theta_v = np.linspace(0, np.pi / 2, ray_count)
        pos_x = np.ones(ray_count) * -2
        s = 80
        lim = (-2, 5, -2.5, 1)
        flags = (0, 0, 1, 0) if user_choice == "3" else (0, 0, 0, 1)
    else:
        raise ValueError("user_choice must be '1', '2', '3' or '4'")
    return (g, ray_count, theta_v, pos_x, s) + lim + flags


# --------------------------------------------------------------------------- step-method tokens (:469-764)
class StepMethod:
    """Token for op<m>.  Passing it to trazar selects the device kernel; calling it advances one ray by
    one DELTA_S step on the device with the reference's argument list (:469)."""

    def __init__(self, m, label):
        self.method = m
        self.__name__ = f"op{m}"
        self.label = label

    def __repr__(self):
        return f"<step method op{self.method}:{self.label}>"

    def __call__(self, i_angle, init_n, i_grad, i_unitv, i_vpos, coef_i, grd, z, step, history=None):
        fld = _field_of(z, grd)
        g = gamma
        st = np.zeros((9, 1))
        st[:, 0] = (i_vpos[0], i_vpos[1], i_angle, init_n, i_grad[0], i_grad[1], 0.0, 0.0, 0.0)
        hist = None
        if self.method == 7:
            if history is None:
                raise ValueError("op7 needs history=[P0, P1] (the two positions before i_vpos; VECTOR_LIST, :73)")
            hist = np.ascontiguousarray(np.asarray(history, dtype=np.float64).reshape(4, 1))
        # one step from a given state has nothing to hand over to a re-trace (rtmi_params.no_retrace)
        b = Batch(fld, self.method, step, max_size=1 << 20, box=(-1e300, 1e300, -1e300, 1e300), gamma=g,
                  thetas=[i_angle], x0=[i_vpos[0]], y0=[i_vpos[1]], record_stride=0, retrace=False)
        b.set_state(st, hist, np.array([3], dtype=np.int32))
        b.step(1)
        fin = b.final()[:, 0]
        b.close()
        return np.array((fin[0], fin[1])), fin[2], fin[3], np.array((fin[4], fin[5]))


_LABELS = ["1st order Taylor + analytical 2-point momentum-impulse", "1st order Taylor + d_theta/d_s Runge-Kutta (AnDF)",
           "2-point curvature + d_theta/d_s Runge-Kutta", "2-point curvature + analytical 2-point momentum-impulse",
           "2-point curvature + optimized 2-point momentum-impulse", "2nd order Taylor + d_theta/d_s Runge-Kutta (HySA)",
           "2nd order Taylor + 4-point difference method (MxSA)", "2nd order Taylor + analytical 2-point momentum-impulse",
           "2nd order Taylor + optimized 2-point momentum-impulse",
           "2-point curvature + optimized anisotropic momentum-impulse",
           "2nd order Taylor + optimized anisotropic momentum-impulse"]
op1, op2, op3, op4, op5, op6, op7, op8, op9, op10, op11 = [StepMethod(i + 1, _LABELS[i]) for i in range(11)]
METHODS = {m.method: m for m in (op1, op2, op3, op4, op5, op6, op7, op8, op9, op10, op11)}
# menus: isotropic scenarios offer 1..9 (:1238-1264), the anisotropic one offers 1..2 -> op10/op11 (:1286-1291)
ISOTROPIC_MENU = {str(i): METHODS[i] for i in range(1, 10)}
ANISOTROPIC_MENU = {"1": op10, "2": op11}


def _method_id(selected_func):
    if isinstance(selected_func, StepMethod):
        return selected_func.method
    if isinstance(selected_func, int) and 1 <= selected_func <= 11:
        return selected_func
    name = getattr(selected_func, "__name__", "")
    if name.startswith("op") and name[2:].isdigit() and 1 <= int(name[2:]) <= 11:
        return int(name[2:])
    raise ValueError(f"selected_func must be one of op1..op11, got {selected_func!r}")


# --------------------------------------------------------------------------- field (:412-464)
class Field:
    """z + grd of interpolacion(), resident in HBM (rtmi_field)."""

    def __init__(self, handle, dtype):
        self._h = C.c_void_p(handle)
        self.dtype = dtype
        qx, qy = C.c_int(), C.c_int()
        check(lib().rtmi_field_dims(self._h, C.byref(qx), C.byref(qy)))
        self.qx, self.qy = qx.value, qy.value

    @classmethod
    def build(cls, scenario, limits=None, delta=DELTA, dtype=F64, stream=None):
        """genZ + interpolacion on the device for one of the four scenarios (rtmi_field_build)."""
        sc = SCENARIOS[scenario] if isinstance(scenario, str) else scenario
        if limits is None:
            limits = constants(USER_CHOICE[scenario])[5:9]
        h = C.c_void_p()
        check(lib().rtmi_field_build(sc.code, *[float(v) for v in limits], float(delta), dtype, stream, C.byref(h)))
        return cls(h.value, dtype)

    @classmethod
    def from_samples(cls, x, y, Z, delta=DELTA, dtype=F64, stream=None):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        if Z.shape != (len(y), len(x)):
            raise ValueError("Z must have shape (len(y), len(x))")
        h = C.c_void_p()
        check(lib().rtmi_field_from_samples(dptr(x), len(x), dptr(y), len(y), dptr(Z), float(delta), dtype, stream,
                                            C.byref(h)))
        return cls(h.value, dtype)

    def arrays(self):
        """(x, y, Z, coef_dy, coef_dx): axes, n samples and the bicubic coefficients of GradX/GradY."""
        x = np.empty(self.qx); y = np.empty(self.qy)
        Z = np.empty((self.qy, self.qx)); cdy = np.empty_like(Z); cdx = np.empty_like(Z)
        check(lib().rtmi_field_read(self._h, dptr(x), dptr(y), dptr(Z), dptr(cdy), dptr(cdx)))
        return x, y, Z, cdy, cdx

    def n_gradient(self, x, y):
        x = np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64)
        y = np.ascontiguousarray(np.atleast_1d(y), dtype=np.float64)
        n = np.empty_like(x); gx = np.empty_like(x); gy = np.empty_like(x)
        check(lib().rtmi_field_eval(self._h, len(x), dptr(x), dptr(y), dptr(n), dptr(gx), dptr(gy)))
        return n, gx, gy

    def lookup_fast(self, x, y):
        """The fast-form step methods' own lookup (the cell's polynomial, rtmi_debug_field_lookup) -> n, dn/dx, dn/dy."""
        x = np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64)
        y = np.ascontiguousarray(np.atleast_1d(y), dtype=np.float64)
        n = np.empty_like(x); gx = np.empty_like(x); gy = np.empty_like(x)
        check(lib().rtmi_debug_field_lookup(self._h, len(x), dptr(x), dptr(y), dptr(n), dptr(gx), dptr(gy)))
        return n, gx, gy

    @property
    def layered(self):
        """1 when the medium depends on y alone and the fast-form fp64 step kernels look it up by the row (rtmi_field_layered)."""
        return int(lib().rtmi_field_layered(self._h))

    def lookup_layered(self, x, y):
        """The lookup of an x-invariant field by its row alone, as the step kernels make it (rtmi_debug_field_lookup_layered)
        -> n, dn/dx (+0), dn/dy.  Raises for a field that is not x-invariant."""
        x = np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64)
        y = np.ascontiguousarray(np.atleast_1d(y), dtype=np.float64)
        n = np.empty_like(x); gx = np.empty_like(x); gy = np.empty_like(x)
        check(lib().rtmi_debug_field_lookup_layered(self._h, len(x), dptr(x), dptr(y), dptr(n), dptr(gx), dptr(gy)))
        return n, gx, gy

    def dgrad(self, x, y):
        """The Jacobian of the gradient as rtmi_paraxial evaluates it (rtmi_field_eval_dgrad): the derivatives of the cell
        polynomials of the two gradient fits -> d(dn/dx)/dx, d(dn/dx)/dy, d(dn/dy)/dx, d(dn/dy)/dy."""
        x = np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64)
        y = np.ascontiguousarray(np.atleast_1d(y), dtype=np.float64)
        out = [np.empty_like(x) for _ in range(4)]
        check(lib().rtmi_field_eval_dgrad(self._h, len(x), dptr(x), dptr(y), *[dptr(o) for o in out]))
        return tuple(out)

    def close(self):
        if self._h:
            lib().rtmi_field_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FieldSpline:
    """One of the three callables interpolacion() returns (z, grd[0], grd[1]); `spl(y, x)` evaluates on
    the device with RectBivariateSpline's argument order and [[value]] return shape (:153-155)."""

    def __init__(self, field, which):
        self.field, self.which = field, which

    def __call__(self, yv, xv):
        n, gx, gy = self.field.n_gradient(np.atleast_1d(xv), np.atleast_1d(yv))
        return {"n": n, "dx": gx, "dy": gy}[self.which].reshape(-1, 1) if np.ndim(xv) else \
            np.array([[{"n": n, "dx": gx, "dy": gy}[self.which][0]]])


def genZ(xi, xs, yi, ys, dtype=F64):
    """RT_bench.py:412-433.  Reads the module-global scenario `f` like the reference.  Returns
    (x, y, X, Y, ZZ) as numpy arrays; ZZ is sampled on the device for the built-in scenarios."""
    if f is None:
        raise RuntimeError("set raytracing_amd.rt_bench.f to a scenario (interface, fisheye, vert_heterogeneous) first")
    qx = int((xs - xi + 6) / DELTA + 1)
    qy = int((ys - yi + 6) / DELTA + 1)
    x, y = np.linspace(xi - 3, xs + 3, qx), np.linspace(yi - 3, ys + 3, qy)
    X, Y = np.meshgrid(x, y)
    if isinstance(f, Scenario):
        fld = Field.build(f, (xi, xs, yi, ys), DELTA, dtype)
        ZZ = fld.arrays()[2]
        fld.close()
    else:
        ZZ = np.asarray(f(X, Y), dtype=np.float64)   # user-supplied n(x, y): sampled by the caller's function
    return x, y, X, Y, ZZ


def interpolacion(x, y, Z, X=None, Y=None, dtype=F64):
    """RT_bench.py:435-464 -> (z, grd, hess).  The fits run on the device; hess is None (the reference
    builds it and never reads it, :462)."""
    fld = Field.from_samples(x, y, Z, DELTA, dtype)
    return FieldSpline(fld, "n"), (FieldSpline(fld, "dy"), FieldSpline(fld, "dx")), None


def _field_of(z, grd=None):
    if isinstance(z, Field):
        return z
    if isinstance(z, FieldSpline):
        return z.field
    raise TypeError("z must come from interpolacion() / Field.build()")


def n_gradient(vector, grd, z):
    """RT_bench.py:141-156."""
    n, gx, gy = _field_of(z, grd).n_gradient(vector[0], vector[1])
    return n[0], np.array([gx[0], gy[0]])


# --------------------------------------------------------------------------- ray batch (:766-948)
class Batch:
    """One trazar() call's rays, resident in HBM (rtmi_batch)."""

    def __init__(self, field, method, step, max_size, box, gamma, thetas, x0, y0, record_stride=1, rec_rows=0,
                 gamma_step=None, stream=None, ext_s_ray=None, ext_n_ray=None, block_size=0, launch_mode="auto",
                 refill_min=0, exact_basis=0, field_path=0, sort_rays=False, lazy_clear=False, keep_n_ray=True, slice_steps=0,
                 reference_order=False, retrace=True):
        self.field = field
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        self.R = len(th)
        x0 = np.ascontiguousarray(np.broadcast_to(np.asarray(x0, dtype=np.float64), (self.R,)))
        y0 = np.ascontiguousarray(np.broadcast_to(np.asarray(y0, dtype=np.float64), (self.R,)))
        p = Params()
        p.method = _method_id(method); p.dtype = field.dtype
        p.gamma = float(gamma); p.gamma_step = float(gamma if gamma_step is None else gamma_step)
        p.step = float(step); p.max_size = int(max_size)
        p.record_stride = int(record_stride); p.rec_rows = int(rec_rows)
        for i in range(4):
            p.box[i] = float(box[i])
        # launch_mode: "auto" (default: the library chooses and, on re-runs, keeps the faster), "plain", "refill", "sliced",
        # or the rtmi_launch_mode integer; results are bit-identical in all of them
        p.launch_mode = LAUNCH_MODES[launch_mode] if isinstance(launch_mode, str) else int(launch_mode)
        p.block_size = int(block_size); p.refill_min = int(refill_min)
        p.exact_basis = int(exact_basis); p.field_path = int(field_path)
        if isinstance(sort_rays, str):
            if sort_rays != "auto":
                raise ValueError("sort_rays must be True, False or 'auto'")
            sort_rays = not launch_is_coherent(x0, y0, th)
        p.sort_rays = int(bool(sort_rays))
        p.ext_s_ray = ext_s_ray; p.ext_n_ray = ext_n_ray
        p.lazy_clear = int(bool(lazy_clear))
        p.no_n_ray = int(not keep_n_ray)
        p.slice_steps = int(slice_steps)
        # rtmi_order: False / 0 default (op7 alone of the fused five steps in the reference's operation order); True / 1 all of
        # op1/2/6/7/8 (fp64: the oracle's bits, slower); "fused" / 2 fused forms throughout, op7 included; "fast_field" / 3 op7's
        # reference-order step on the fused field lookup
        p.reference_order = ORDERS[reference_order] if isinstance(reference_order, str) else int(reference_order)
        # retrace (default on): a fused fp64 op1/2/6/8 batch re-traces its critical rays -- those running along a sharp
        # transition of the medium -- in reference order by itself (rtmi_params.no_retrace)
        p.no_retrace = int(not retrace)
        self.params = p
        self._h = C.c_void_p()
        check(lib().rtmi_batch_create(field._h, C.byref(p), self.R, dptr(x0), dptr(y0), dptr(th), stream,
                                      C.byref(self._h)))
        self.max_size = int(max_size)
        self.record_stride = int(record_stride)
        self.rec_rows = int(rec_rows) if rec_rows else ((self.max_size + record_stride - 1) // record_stride
                                                        if record_stride else 0)

    def set_state(self, state9, hist4=None, istep=None):
        st = np.ascontiguousarray(state9, dtype=np.float64)
        assert st.shape == (9, self.R)
        h = np.ascontiguousarray(hist4, dtype=np.float64) if hist4 is not None else None
        i = np.ascontiguousarray(istep, dtype=np.int32) if istep is not None else None
        check(lib().rtmi_batch_set_state(self._h, dptr(st), dptr(h), i.ctypes.data_as(_lib._ip) if i is not None else None))

    def get_state(self):
        """(state9 [9,R], aux4 [4,R], istep [R], alive [R]) -- rtmi_batch_get_state; restore_state(*get_state()) on a batch
        with the same parameters resumes bit for bit."""
        st = np.empty((9, self.R)); h = np.empty((4, self.R)); i = np.empty(self.R, dtype=np.int32)
        al = np.empty(self.R, dtype=np.uint8)
        check(lib().rtmi_batch_get_state(self._h, dptr(st), dptr(h), i.ctypes.data_as(_lib._ip), al.ctypes.data))
        return st, h, i, al

    def restore_state(self, state9, aux4, istep, alive):
        st = np.ascontiguousarray(state9, dtype=np.float64)
        h = np.ascontiguousarray(aux4, dtype=np.float64)
        i = np.ascontiguousarray(istep, dtype=np.int32)
        al = np.ascontiguousarray(alive, dtype=np.uint8)
        assert st.shape == (9, self.R) and h.shape == (4, self.R) and i.shape == (self.R,) and al.shape == (self.R,)
        check(lib().rtmi_batch_restore_state(self._h, dptr(st), dptr(h), i.ctypes.data_as(_lib._ip), al.ctypes.data))

    def set_per_ray(self, step, max_size):
        """Per-ray DELTA_S and max_size ([R] each, caller's ray order): rtmi_batch_set_per_ray."""
        st = np.ascontiguousarray(np.broadcast_to(np.asarray(step, dtype=np.float64), (self.R,)))
        ms = np.ascontiguousarray(np.broadcast_to(np.asarray(max_size, dtype=np.int32), (self.R,)))
        check(lib().rtmi_batch_set_per_ray(self._h, dptr(st), ms.ctypes.data_as(_lib._ip)))

    def reset(self):
        check(lib().rtmi_batch_reset(self._h))

    def step(self, nsteps=1, count=1):
        """Advance every live ray by nsteps DELTA_S steps; count > 1: that many such launches as one hipGraph."""
        if count > 1:
            check(lib().rtmi_step_repeat(self._h, int(nsteps), int(count)))
        else:
            check(lib().rtmi_step(self._h, int(nsteps)))

    def run(self):
        check(lib().rtmi_run(self._h))

    def sync(self):
        check(lib().rtmi_sync(self._h))

    def d_ray(self):
        d = np.empty((3, self.R))
        check(lib().rtmi_read_d_ray(self._h, dptr(d)))
        return d

    def final(self):
        out = np.empty((9, self.R))
        check(lib().rtmi_read_final(self._h, dptr(out)))
        return out

    def rows(self, row0=0, nrows=None, want_n_ray=False):
        nrows = self.rec_rows - row0 if nrows is None else nrows
        s = np.empty((nrows, 6, self.R))
        n = np.empty((nrows, self.R)) if want_n_ray else None
        check(lib().rtmi_read_rows(self._h, row0, nrows, dptr(s), dptr(n)))
        return (s, n) if want_n_ray else s

    def metric(self, kind):
        """On-device per-ray metric: "snell" (degrees), "closure" (%), "px_cv" (%); see rtmi_metric."""
        out = np.empty(self.R)
        check(lib().rtmi_metric(self._h, {"snell": 1, "closure": 2, "px_cv": 3}[kind], dptr(out)))
        return out

    def isochrones(self, times):
        """(x, y, theta) of every ray at the given traveltimes -> [ntimes, 3, R], NaN where not reached."""
        t = np.ascontiguousarray(times, dtype=np.float64)
        out = np.empty((len(t), 3, self.R))
        check(lib().rtmi_isochrones(self._h, len(t), dptr(t), dptr(out)))
        return out

    def crossings(self, line, kmax=4):
        """Where each recorded ray crosses the line a x + b y = c (line = (a, b, c)): rtmi_crossings.  Returns a dict with
        count [R] (crossings per ray, -1 when the trajectory reaches past the record) and u, x, y, T, theta, s [kmax, R]
        (u the coordinate along the line, s the fractional step; NaN past count).  Needs record_stride 1."""
        ln = np.ascontiguousarray(line, dtype=np.float64)
        if ln.shape != (3,):
            raise ValueError("line must be (a, b, c)")
        count = np.empty(self.R, dtype=np.int32)
        out = np.empty((int(kmax), 6, self.R))
        check(lib().rtmi_crossings(self._h, dptr(ln), int(kmax), count.ctypes.data_as(_lib._ip), dptr(out)))
        d = {"count": count}
        for q, k in enumerate(CROSSING_FIELDS):
            d[k] = out[:, q].copy()
        return d

    def paraxial(self, line=None, kmax=4):
        """Dynamic ray tracing along the recorded rays (rtmi_paraxial): the plane-wave (Q1, P1) and point-source (Q2, P2)
        solutions of the paraxial system, the spread J = n0 Q2 per radian of launch angle, the spreading factor
        G = (n |J|)^-1/2 and the caustic count kmah.  Returns a dict of [R] arrays Q1, P1, Q2, P2, J, G, kmah at the end of each
        ray (NaN for a ray whose trajectory reaches past the record); with a line (a, b, c) also count [R] (rtmi_crossings')
        and 'at_line', a dict of the same seven as [kmax, R] arrays at the crossings (NaN past count).  Needs record_stride 1,
        op1..op9 and gamma 1."""
        end = np.empty((len(PARAXIAL_FIELDS), self.R))
        if line is None:
            check(lib().rtmi_paraxial(self._h, None, 0, None, None, dptr(end)))
            return {k: end[q].copy() for q, k in enumerate(PARAXIAL_FIELDS)}
        ln = np.ascontiguousarray(line, dtype=np.float64)
        if ln.shape != (3,):
            raise ValueError("line must be (a, b, c)")
        count = np.empty(self.R, dtype=np.int32)
        at = np.empty((int(kmax), len(PARAXIAL_FIELDS), self.R))
        check(lib().rtmi_paraxial(self._h, dptr(ln), int(kmax), count.ctypes.data_as(_lib._ip), dptr(at), dptr(end)))
        d = {k: end[q].copy() for q, k in enumerate(PARAXIAL_FIELDS)}
        d["count"] = count
        d["at_line"] = {k: at[:, q].copy() for q, k in enumerate(PARAXIAL_FIELDS)}
        return d

    def first_arrival_grid(self, grid, fan_size=None, max_gap=None, max_dtheta=None, amplitude=False, stats=False):
        """First-arrival traveltime table on a regular grid from the recorded fans (rtmi_first_arrival_grid): the batch's rays
        are R / fan_size fans of fan_size rays each (default: one fan), ordered by launch angle.  grid = (gx0, gdx, nx, gy0,
        gdy, ny): node (ix, iy) at (gx0 + ix gdx, gy0 + iy gdy).  max_gap / max_dtheta: the gap rule (None: the library's
        defaults, 8 grid spacings and 0.25 rad).  Returns a dict of [S, ny, nx] arrays: count (arrival branches covering the
        node) and T, theta0, theta, ray, step of the first arrival (NaN where count is 0); with amplitude=True also J, G, kmah
        (op1..op9, gamma 1); with stats=True also 'stats'.  Needs record_stride 1."""
        M = self.R if fan_size is None else int(fan_size)
        return _grid_call(lambda gp, cnt, out, st: lib().rtmi_first_arrival_grid(self._h, M, gp, cnt, out, st),
                          self.R // M if M >= 1 else 0, grid, max_gap, max_dtheta, amplitude, stats)

    def arrival_grid(self, grid, arrivals=1, order="time", fan_size=None, max_gap=None, max_dtheta=None, amplitude=False, stats=False,
                     count_only=False):
        """The `arrivals` first arrivals per node of the recorded fans (rtmi_arrival_grid), by order "time" (the earliest) or
        "amplitude" (the most energetic first: the least n |J|; op1..op9, gamma 1).  Arguments as first_arrival_grid.  Returns
        its dict with arrays of shape [S, arrivals, ny, nx], NaN past a node's count; count is [S, ny, nx].  stats adds
        'candidates' (the sum of count) and 'scan_ms'.  count_only: count (and stats) alone, before the candidate list exists."""
        M = self.R if fan_size is None else int(fan_size)
        return _arrival_call(lambda gp, ap, cnt, out, st: lib().rtmi_arrival_grid(self._h, M, gp, ap, cnt, out, st),
                             self.R // M if M >= 1 else 0, grid, arrivals, order, max_gap, max_dtheta, amplitude, stats, count_only)

    def gaussian_beams(self, grid, omegas, eps, fan_size=None, cutoff=None, max_width=None, edge_taper=0, stats=False):
        """Gaussian beam summation (rtmi_gaussian_beams): the frequency-domain wavefield of each fan's source at every node of
        grid = (gx0, gdx, nx, gy0, gdy, ny), summed over the fan's beams.  The batch's rays are R / fan_size fans (default: one),
        each with strictly monotone launch angles.  omegas: the frequencies; eps: the beam parameter (narrowest beams at
        distance D for eps ~ D / n0); cutoff / max_width: None takes the library's defaults (18, 64 grid spacings); edge_taper:
        radians of cosine taper at both ends of each fan.  Returns complex128 [S, nw, ny, nx]; with stats=True (u, stats).
        Needs record_stride 1, op1..op9 and gamma 1."""
        M = self.R if fan_size is None else int(fan_size)
        return _beam_call(lambda bp, nw, om, u, st: lib().rtmi_gaussian_beams(self._h, M, bp, nw, om, u, st),
                          self.R // M if M >= 1 else 0, grid, omegas, eps, cutoff, max_width, edge_taper, stats)

    def traveltime_perturb(self, dZ, line=None, kmax=4, stats=False):
        """The Frechet derivative of the reported traveltimes applied to a change dZ [qy, qx] of the field's n samples, the rows
        held fixed (rtmi_traveltime_perturb): returns {"end": [R], "line": [kmax, R], "count": [R]} -- the change of each ray's
        traveltime at its end (NaN past the record) and at its crossings of the line (a, b, c) (NaN past count; without a line
        "line" is [0, R] and "count" is None); with stats=True also 'stats'.  Needs record_stride 1."""
        qx, qy = self.field.qx, self.field.qy
        dz = np.ascontiguousarray(dZ, dtype=np.float64)
        if dz.shape != (qy, qx):
            raise ValueError(f"dZ must have shape ({qy}, {qx})")
        end = np.empty(self.R)
        st = _lib.SensitivityStats()
        if line is None:
            check(lib().rtmi_traveltime_perturb(self._h, None, 0, dptr(dz), None, None, dptr(end), C.byref(st)))
            d = {"end": end, "line": np.empty((0, self.R)), "count": None}
        else:
            ln = np.ascontiguousarray(line, dtype=np.float64)
            if ln.shape != (3,):
                raise ValueError("line must be (a, b, c)")
            count = np.empty(self.R, dtype=np.int32)
            out = np.empty((max(int(kmax), 0), self.R))
            check(lib().rtmi_traveltime_perturb(self._h, dptr(ln), int(kmax), dptr(dz), count.ctypes.data_as(_lib._ip), dptr(out),
                                                dptr(end), C.byref(st)))
            d = {"end": end, "line": out, "count": count}
        if stats:
            d["stats"] = sensitivity_stats(st)
        return d

    def traveltime_backproject(self, w_end=None, w_line=None, line=None, kmax=4, stats=False):
        """The transpose (rtmi_traveltime_backproject): weights w_end [R] on the ray ends and / or w_line [kmax, R] on the
        crossings of the line (a, b, c) -> g [qy, qx] on the field's n samples, with <A dZ, w> = <dZ, g>.  NaN or absent
        weights count as 0.  The result has the same bits in every schedule, ray sorting and ray order.  With stats=True returns
        (g, stats)."""
        we = None if w_end is None else np.ascontiguousarray(w_end, dtype=np.float64)
        if we is not None and we.shape != (self.R,):
            raise ValueError(f"w_end must have shape ({self.R},)")
        wl = None if w_line is None else np.ascontiguousarray(w_line, dtype=np.float64)
        if wl is not None and wl.shape != (int(kmax), self.R):
            raise ValueError(f"w_line must have shape ({int(kmax)}, {self.R})")
        ln = None
        if line is not None:
            ln = np.ascontiguousarray(line, dtype=np.float64)
            if ln.shape != (3,):
                raise ValueError("line must be (a, b, c)")
        g = np.empty((self.field.qy, self.field.qx))
        st = _lib.SensitivityStats()
        check(lib().rtmi_traveltime_backproject(self._h, None if ln is None else dptr(ln), int(kmax) if ln is not None else 0,
                                                None if wl is None else dptr(wl), None if we is None else dptr(we), dptr(g),
                                                C.byref(st)))
        return (g, sensitivity_stats(st)) if stats else g

    def paraxial_rows(self):
        """J and kmah after every recorded row ([rec_rows, R] each; NaN / -1 past a ray's end): rtmi_debug_paraxial_rows."""
        v = self.view()
        J = np.empty((int(v.rec_rows), self.R))
        km = np.empty((int(v.rec_rows), self.R), dtype=np.int32)
        check(lib().rtmi_debug_paraxial_rows(self._h, dptr(J), km.ctypes.data_as(_lib._ip)))
        return J, km

    def wavefronts(self, times, nfine=100):
        """The reference's wavefront extraction (RT_bench.py:1005-1044) on the device: one dict per traveltime with the
        points of the wavefront sorted by y -- 'y', 'x', 'angle' (ray angle), 'dxdy' (derivative of the PCHIP interpolant
        x(y) at the points), 'normal' (normal angle), 'angle_diff' (|ray angle - normal angle|), 'ray' (ray indices) --
        and 'x_fine', 'y_fine' (the interpolated wavefront on nfine points).  Wavefronts with < 2 points have empty
        derived arrays, like the reference, which skips them (:1011); one with two points of equal y (scipy raises) has NaN
        throughout its derived arrays."""
        t = np.ascontiguousarray(times, dtype=np.float64)
        nt = len(t)
        count = np.zeros(nt, dtype=np.int64)
        nodes = np.empty((nt, 7, self.R))
        fine = np.empty((nt, 2, nfine)) if nfine else None
        check(lib().rtmi_wavefronts(self._h, nt, dptr(t), int(nfine), count.ctypes.data_as(C.POINTER(C.c_int64)), dptr(nodes),
                                    dptr(fine)))
        out = []
        for i in range(nt):
            n = int(count[i])
            d = dict(time=float(t[i]), count=n, y=nodes[i, 0, :n].copy(), x=nodes[i, 1, :n].copy(), angle=nodes[i, 2, :n].copy(),
                     ray=nodes[i, 6, :n].astype(np.int64))
            m = n if n >= 2 else 0
            d.update(dxdy=nodes[i, 3, :m].copy(), normal=nodes[i, 4, :m].copy(), angle_diff=nodes[i, 5, :m].copy(),
                     x_fine=fine[i, 0].copy() if nfine and m else np.empty(0), y_fine=fine[i, 1].copy() if nfine and m else np.empty(0))
            out.append(d)
        return out

    def stats(self):
        s = Stats()
        check(lib().rtmi_batch_stats(self._h, C.byref(s)))
        out = {k: getattr(s, k) for k, _ in Stats._fields_ if not k.startswith("auto_") and k != "reserved_"}     # incl. retraced, retrace_overflow, dispatch_first
        out["launch_mode_used"] = LAUNCH_NAMES.get(out["launch_mode_used"], out["launch_mode_used"])
        out["auto_fallbacks"] = s.auto_fallbacks
        # RTMI_LAUNCH_AUTO's exploration record: kernel ms of each timed run per schedule, and the schedule kept (None: still exploring / no choice)
        out["auto_exploration"] = {"sliced_ms": [s.auto_ms[0][i] for i in range(s.auto_n[0])],
                                   "plain_ms": [s.auto_ms[1][i] for i in range(s.auto_n[1])],
                                   "kept": LAUNCH_NAMES.get(s.auto_kept) if s.auto_kept else None}
        return out

    def view(self):
        v = DeviceView()
        check(lib().rtmi_batch_view(self._h, C.byref(v)))
        return v

    def device_tensors(self):
        """Zero-copy torch views of the batch's device memory (rtmi_batch_view through
        __cuda_array_interface__): SoA state [R], istep [R], s_ray [rec_rows, 6, R], n_ray [rec_rows, R].
        For consumers that stay on the GPU or feed torch.distributed (RCCL) collectives; the tensors alias
        library memory and die with the batch."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("torch sees no HIP device (raytracing_amd._lib maps torch's own HIP runtime before librtmi.so so "
                               "that the two share one; RTMI_NO_PRELOAD=1 or an RTMI_LIB_PATH build linked elsewhere defeats that)")
        v = self.view()
        ts = "<f8" if v.dtype == F64 else "<f4"

        class _Cai:
            def __init__(self, ptr, shape, typestr):
                self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False),
                                                 "version": 2, "strides": None}
        dev = torch.device("cuda", torch.cuda.current_device())
        # accumulated quantities are fp64 in both precisions (rtmi_device_view); n and its gradient are of the dtype
        out = {name: torch.as_tensor(_Cai(getattr(v, name), (self.R,), "<f8" if name in _ACC else ts), device=dev)
               for name in ("x", "y", "theta", "n", "gx", "gy", "dist_sim", "dist_real", "T")}
        out["istep"] = torch.as_tensor(_Cai(v.istep, (self.R,), "<i4"), device=dev)
        if v.perm:   # sort_rays: slot k of every tensor here is the caller's ray perm[k]
            out["perm"] = torch.as_tensor(_Cai(v.perm, (self.R,), "<i4"), device=dev)
        if v.s_ray:
            out["s_ray"] = torch.as_tensor(_Cai(v.s_ray, (int(v.rec_rows), 6, self.R), ts), device=dev)
        if v.n_ray:
            out["n_ray"] = torch.as_tensor(_Cai(v.n_ray, (int(v.rec_rows), self.R), ts), device=dev)
        return out

    def close(self):
        if self._h:
            lib().rtmi_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Shard:
    """One trazar() call's rays over several GPUs of this node from ONE process (rtmi_shard, include/rtmi.h): rays dealt to
    `devices` round-robin, each device builds the field and runs its rays, the read-back gathers to devices[0] device to device
    (transport "auto" | "rccl" | "copy").  Listing one device several times rehearses the split on a single GPU (copies)."""

    def __init__(self, scenario, method, step, max_size, box, gamma, thetas, x0, y0, devices, limits=None, delta=DELTA, dtype=F64,
                 record_stride=1, rec_rows=0, transport="auto", gamma_step=None, launch_mode="auto", reference_order=False,
                 keep_n_ray=False):
        sc = SCENARIOS[scenario] if isinstance(scenario, str) else scenario
        if limits is None:
            limits = constants(USER_CHOICE[scenario])[5:9]
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        self.R = len(th)
        x0 = np.ascontiguousarray(np.broadcast_to(np.asarray(x0, dtype=np.float64), (self.R,)))
        y0 = np.ascontiguousarray(np.broadcast_to(np.asarray(y0, dtype=np.float64), (self.R,)))
        p = Params()
        p.method = _method_id(method); p.dtype = dtype
        p.gamma = float(gamma); p.gamma_step = float(gamma if gamma_step is None else gamma_step)
        p.step = float(step); p.max_size = int(max_size); p.record_stride = int(record_stride); p.rec_rows = int(rec_rows)
        for i in range(4):
            p.box[i] = float(box[i])
        p.launch_mode = LAUNCH_MODES[launch_mode] if isinstance(launch_mode, str) else int(launch_mode)
        p.no_n_ray = int(not keep_n_ray)
        p.reference_order = ORDERS[reference_order] if isinstance(reference_order, str) else int(reference_order)
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        self.devices = [int(d) for d in dev]
        self._h = C.c_void_p()
        check(lib().rtmi_shard_create(sc.code, *[float(v) for v in limits], float(delta), C.byref(p), self.R, dptr(x0), dptr(y0), dptr(th),
                                      dev.ctypes.data_as(_lib._ip), len(dev), {"auto": 0, "rccl": 1, "copy": 2}[transport],
                                      C.byref(self._h)))

    def run(self):
        check(lib().rtmi_shard_run(self._h))

    def reset(self):
        check(lib().rtmi_shard_reset(self._h))

    def d_ray(self):
        d = np.empty((3, self.R))
        check(lib().rtmi_shard_read_d_ray(self._h, dptr(d)))
        return d

    def final(self):
        out = np.empty((9, self.R))
        check(lib().rtmi_shard_read_final(self._h, dptr(out)))
        return out

    def rows(self, row0, nrows, every=1):
        s = np.empty((nrows, 6, self.R))
        check(lib().rtmi_shard_read_rows(self._h, int(row0), int(nrows), int(every), dptr(s)))
        return s

    def info(self):
        st = _lib.ShardStats()
        check(lib().rtmi_shard_info(self._h, C.byref(st)))
        out = {k: getattr(st, k) for k, _ in _lib.ShardStats._fields_ if k != "reserved_"}
        out["transport"] = {1: "rccl", 2: "copy"}.get(out["transport"], out["transport"])
        return out

    def close(self):
        if self._h:
            lib().rtmi_shard_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


CROSSING_FIELDS = ("u", "x", "y", "T", "theta", "s")                            # rtmi_crossings' out[kmax][6][R]
ARRIVAL_FIELDS = ("theta0", "T", "u", "x", "y", "theta", "residual", "iterations", "status")   # rtmi_two_point's arrivals[..][9]
PARAXIAL_FIELDS = ("Q1", "P1", "Q2", "P2", "J", "G", "kmah")                     # rtmi_paraxial's [7] columns


def two_point(selected_func, field, sources, line, receivers_u, *, thetas, step, max_size, box, gamma=1, reference_order=False,
              retrace=True, tol=1e-10, max_arrivals=4, max_crossings=4, max_iter=60, mem_budget=0, gamma_step=None,
              launch_mode="auto", field_path=0, stats=False, paraxial=False, sensitivity=False):
    """Rays from each source to each receiver on the line a x + b y = c (line = (a, b, c)), all on the device
    (rtmi_two_point): a fan of launch angles `thetas` per source, brackets between adjacent fan rays, Illinois regula falsi on
    the launch angle.  sources: (S, 2) array of (x, y); receivers_u: [J] coordinates along the line (u = a' y - b' x with
    (a', b') the unit normal), strictly increasing.  Returns a dict of [S, J, A] arrays -- theta0 (launch angle), T, u, x, y,
    theta (angle at the receiver), residual (u - u_j), iterations, status (rtmi_arrival_status) -- with the converged
    arrivals first, sorted by T; count [S, J] (converged arrivals) and nbad [S, J] (stalled or truncated brackets); with
    stats=True also 'stats' (iterations, groups, rec_rows, overflow, fan_ms, bracket_ms, refine_ms).  With paraxial=True also
    [S, J, A] arrays Q2, P2, J, G, kmah of the converged arrivals (NaN elsewhere): _two_point_paraxial.  With sensitivity=True
    also 'sensitivity', a TravelTimeSensitivity over the converged arrivals (close() it when done)."""
    src = np.ascontiguousarray(np.asarray(sources, dtype=np.float64).reshape(-1, 2))
    sx = np.ascontiguousarray(src[:, 0]); sy = np.ascontiguousarray(src[:, 1])
    th = np.ascontiguousarray(thetas, dtype=np.float64)
    ru = np.ascontiguousarray(receivers_u, dtype=np.float64)
    ln = np.ascontiguousarray(line, dtype=np.float64)
    if ln.shape != (3,):
        raise ValueError("line must be (a, b, c)")
    S, M, J, A = len(sx), len(th), len(ru), int(max_arrivals)
    p = Params()
    p.method = _method_id(selected_func); p.dtype = field.dtype
    p.gamma = float(gamma); p.gamma_step = float(gamma if gamma_step is None else gamma_step)
    p.step = float(step); p.max_size = int(max_size)
    for i in range(4):
        p.box[i] = float(box[i])
    p.launch_mode = LAUNCH_MODES[launch_mode] if isinstance(launch_mode, str) else int(launch_mode)
    p.field_path = int(field_path)
    p.reference_order = ORDERS[reference_order] if isinstance(reference_order, str) else int(reference_order)
    p.no_retrace = int(not retrace)
    tp = _lib.TwoPointParams()
    tp.max_arrivals = A; tp.max_crossings = int(max_crossings); tp.max_iter = int(max_iter); tp.tol = float(tol)
    tp.mem_budget = int(mem_budget)
    count = np.empty((S, J), dtype=np.int32); nbad = np.empty((S, J), dtype=np.int32)
    arr = np.empty((S, J, A, len(ARRIVAL_FIELDS)))
    st = _lib.TwoPointStats()
    check(lib().rtmi_two_point(field._h, C.byref(p), S, dptr(sx), dptr(sy), M, dptr(th), dptr(ln), J, dptr(ru), C.byref(tp),
                               count.ctypes.data_as(_lib._ip), nbad.ctypes.data_as(_lib._ip), dptr(arr), C.byref(st)))
    out = {k: arr[..., q].copy() for q, k in enumerate(ARRIVAL_FIELDS)}
    out["iterations"] = np.nan_to_num(out["iterations"], nan=0.0).astype(np.int32)      # empty slots: 0
    out["status"] = out["status"].astype(np.int32)
    out["count"] = count
    out["nbad"] = nbad
    if stats:
        out["stats"] = {k: getattr(st, k) for k, _ in _lib.TwoPointStats._fields_ if k != "reserved"}
    if paraxial:
        out.update(_two_point_paraxial(field, p, sx, sy, ln, out, int(max_crossings)))
    if sensitivity:
        out["sensitivity"] = TravelTimeSensitivity(field, p, sx, sy, ln, out, int(max_crossings))
    return out


def sensitivity_stats(st):
    return {"kernel_ms": st.kernel_ms, "atomics": int(st.atomics), "scale_exp": int(st.scale_exp)}


class TravelTimeSensitivity:
    """The Frechet derivative of two_point's converged arrival traveltimes with respect to the field's n samples Z [qy, qx]
    (the ray-tomography Jacobian, rays held fixed), built by public calls only, as _two_point_paraxial is: one fresh batch of
    the converged (source, launch angle) rays with the solver's parameters -- sized by a count pass --, kept alive here; each
    arrival takes the crossing whose u and T are bit-equal to its own.  index [n_arrivals, 3]: the (s, j, a) of each row;
    shape = (n_arrivals, qy * qx); matvec(dZ) -> dT [n_arrivals], rmatvec(r) -> g [qy * qx]; as_linear_operator() for
    scipy.sparse.linalg (lsqr); close() frees the batch."""

    def __init__(self, field, p, sx, sy, line, arr, kmax):
        self.field = field
        self.line = np.ascontiguousarray(line, dtype=np.float64)
        self.kmax = int(kmax)
        self.index = np.argwhere(arr["status"] == _lib.ARRIVAL_CONVERGED)
        self.shape = (len(self.index), field.qy * field.qx)
        self._h = None
        R = len(self.index)
        self._rays = R
        if R == 0:
            self._cross = np.zeros(0, dtype=np.int64)
            return
        x0 = np.ascontiguousarray(sx[self.index[:, 0]]); y0 = np.ascontiguousarray(sy[self.index[:, 0]])
        th = np.ascontiguousarray(arr["theta0"][tuple(self.index.T)])
        q = Params.from_buffer_copy(p)
        q.sort_rays = 0; q.no_n_ray = 1; q.lazy_clear = 0; q.ext_s_ray = None; q.ext_n_ray = None

        def batch(stride, rows):
            q.record_stride = stride; q.rec_rows = rows
            h = C.c_void_p()
            check(lib().rtmi_batch_create(field._h, C.byref(q), R, dptr(x0), dptr(y0), dptr(th), None, C.byref(h)))
            return h
        h = batch(0, 0)
        try:
            check(lib().rtmi_run(h))
            d = np.empty((3, R))
            check(lib().rtmi_read_d_ray(h, dptr(d)))
        finally:
            lib().rtmi_batch_destroy(h)
        self._h = batch(1, int(d[2].max()) + 1)
        check(lib().rtmi_run(self._h))
        cnt = np.empty(R, dtype=np.int32)
        cr = np.empty((self.kmax, len(CROSSING_FIELDS), R))
        check(lib().rtmi_crossings(self._h, dptr(self.line), self.kmax, cnt.ctypes.data_as(_lib._ip), dptr(cr)))
        iu, iT = CROSSING_FIELDS.index("u"), CROSSING_FIELDS.index("T")
        self._cross = np.empty(R, dtype=np.int64)
        for r, (s_, j, a) in enumerate(self.index):
            hit = np.nonzero((cr[:, iu, r] == arr["u"][s_, j, a]) & (cr[:, iT, r] == arr["T"][s_, j, a]))[0]
            if len(hit) == 0:
                self.close()
                raise RuntimeError(f"two_point: no crossing of the re-traced ray matches arrival {(s_, j, a)}")
            self._cross[r] = hit[0]

    def matvec(self, dZ):
        """dT [n_arrivals] of the converged arrivals for dZ ([qy, qx] or flat [qy * qx])"""
        if self._rays == 0:
            return np.zeros(0)
        dz = np.asarray(dZ, dtype=np.float64).reshape(self.field.qy, self.field.qx)
        out = np.empty((self.kmax, self._rays))
        cnt = np.empty(self._rays, dtype=np.int32)
        end = np.empty(self._rays)
        check(lib().rtmi_traveltime_perturb(self._h, dptr(self.line), self.kmax, dptr(np.ascontiguousarray(dz)),
                                            cnt.ctypes.data_as(_lib._ip), dptr(out), dptr(end), None))
        return out[self._cross, np.arange(self._rays)].copy()

    def rmatvec(self, r):
        """g [qy * qx] = A^T r for residuals r [n_arrivals]"""
        if self._rays == 0:
            return np.zeros(self.shape[1])
        w = np.zeros((self.kmax, self._rays))
        w[self._cross, np.arange(self._rays)] = np.asarray(r, dtype=np.float64).reshape(-1)
        g = np.empty((self.field.qy, self.field.qx))
        check(lib().rtmi_traveltime_backproject(self._h, dptr(self.line), self.kmax, dptr(w), None, dptr(g), None))
        return g.reshape(-1)

    def as_linear_operator(self):
        from scipy.sparse.linalg import LinearOperator
        return LinearOperator(self.shape, matvec=self.matvec, rmatvec=self.rmatvec, dtype=np.float64)

    def close(self):
        if self._h:
            lib().rtmi_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tomo_stats(st):
    return {k: getattr(st, k) for k, _ in _lib.TomoStats._fields_ if not k.startswith("reserved")}


class Tomography:
    """Recorded rays compiled into a sparse ray-tomography matrix on the device (rtmi_tomo_*): the Jacobian of reported
    traveltimes with respect to the field's n samples Z [qy, qx], one row per observation.  The handle keeps the matrix, not the
    record: after append the batch may be closed, so a joint inversion appends source after source.  shape = (rows, qy * qx)."""

    def __init__(self, field):
        self.qx, self.qy = field.qx, field.qy
        self._h = None
        h = C.c_void_p()
        check(lib().rtmi_tomo_create(field._h, C.byref(h)))
        self._h = h

    def _open(self):
        if not self._h:
            raise ValueError("Tomography: the handle is closed")
        return self._h

    @property
    def shape(self):
        return (self.info()["rows"], self.qy * self.qx)

    def _append(self, batch_handle, R, which, line, kmax):
        wh = None
        if which is not None:
            wh = np.ascontiguousarray(which, dtype=np.int32)
            if wh.shape != (R,):
                raise ValueError(f"which must have shape ({R},)")
        ln = None
        if line is not None:
            ln = np.ascontiguousarray(line, dtype=np.float64)
            if ln.shape != (3,):
                raise ValueError("line must be (a, b, c)")
        nseg = np.empty(R, dtype=np.int32)
        first = C.c_int64()
        check(lib().rtmi_tomo_append(self._open(), batch_handle, None if ln is None else dptr(ln), int(kmax) if ln is not None else 0,
                                     None if wh is None else wh.ctypes.data_as(_lib._ip), nseg.ctypes.data_as(_lib._ip), C.byref(first)))
        return int(first.value), nseg

    def append(self, batch, which=None, line=None, kmax=4):
        """One row per ray of `batch` (record_stride 1), in the caller's ray order: which [R] selects ray m's observation, -1 its
        end, c >= 0 crossing c of line (a, b, c), _lib.TOMO_SKIP no row; None: every ray's end.  Returns (first_row, nseg [R]:
        the row's segments, 0 for an empty row, -1 for a skipped ray).  The batch may be closed afterwards."""
        return self._append(batch._h, batch.R, which, line, kmax)

    def append_sensitivity(self, sens, rows=None):
        """The arrivals of a TravelTimeSensitivity (two_point(..., sensitivity=True)) as rows, in its order; rows: only these
        arrivals (indices into sens.index, ascending).  sens.close() is safe afterwards."""
        if sens._rays == 0:
            return self.info()["rows"], np.zeros(0, dtype=np.int32)
        if not sens._h:
            raise ValueError("Tomography.append_sensitivity: the sensitivity is closed")
        which = np.asarray(sens._cross, dtype=np.int32)
        if rows is not None:
            keep = np.zeros(sens._rays, dtype=bool)
            keep[np.asarray(rows, dtype=np.int64)] = True
            which = np.where(keep, which, _lib.TOMO_SKIP).astype(np.int32)
        return self._append(sens._h, sens._rays, which, sens.line, sens.kmax)

    def info(self):
        st = _lib.TomoStats()
        check(lib().rtmi_tomo_info(self._open(), C.byref(st)))
        return tomo_stats(st)

    def matvec(self, x, stats=False):
        """y [rows] = A x for x [qy, qx] (or flat), one fixed summation order"""
        xx = np.ascontiguousarray(x, dtype=np.float64)
        if xx.size != self.qy * self.qx:
            raise ValueError(f"Tomography.matvec: x must have {self.qy * self.qx} values")
        y = np.empty(self.info()["rows"])
        st = _lib.TomoStats()
        check(lib().rtmi_tomo_apply(self._open(), dptr(xx), dptr(y), C.byref(st)))
        return (y, tomo_stats(st)) if stats else y

    def rmatvec(self, w, stats=False):
        """g [qy, qx] = A^T w for w [rows]: the same bits in every schedule, order of appends and order of rays"""
        ww = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
        if ww.size != self.info()["rows"]:
            raise ValueError(f"Tomography.rmatvec: w must have {self.info()['rows']} values")
        g = np.empty((self.qy, self.qx))
        st = _lib.TomoStats()
        check(lib().rtmi_tomo_transpose(self._open(), dptr(ww), dptr(g), C.byref(st)))
        return (g, tomo_stats(st)) if stats else g

    def _device_tensor(self, who, t, name):
        import torch
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{type(self).__name__}.{who}: {name} must be a torch tensor")
        if t.dtype != torch.float64:
            raise TypeError(f"{type(self).__name__}.{who}: {name} must be float64")
        if not t.is_contiguous():
            raise ValueError(f"{type(self).__name__}.{who}: {name} must be contiguous")
        if not t.is_cuda:                              # which GPU it is on, and its length, the library checks
            raise ValueError(f"{type(self).__name__}.{who}: {name} must be a tensor on a GPU, not on the host")
        return t

    def matvec_device(self, x, out=None, stats=False):
        """rtmi_tomo_apply_dev on torch tensors of the handle's device: x [qy, qx] -> y [rows] (out, if given)"""
        import torch
        self._device_tensor("matvec_device", x, "x")
        y = torch.empty(self.info()["rows"], dtype=torch.float64, device=x.device) if out is None else self._device_tensor("matvec_device", out, "out")
        st = _lib.TomoStats()
        torch.cuda.synchronize(x.device)               # the library works on the null stream
        check(lib().rtmi_tomo_apply_dev(self._open(), x.data_ptr(), y.data_ptr(), C.byref(st)))
        return (y, tomo_stats(st)) if stats else y

    def rmatvec_device(self, w, out=None, stats=False):
        """rtmi_tomo_transpose_dev on torch tensors of the handle's device: w [rows] -> g [qy, qx] (out, if given)"""
        import torch
        self._device_tensor("rmatvec_device", w, "w")
        g = torch.empty((self.qy, self.qx), dtype=torch.float64, device=w.device) if out is None else self._device_tensor("rmatvec_device", out, "out")
        st = _lib.TomoStats()
        torch.cuda.synchronize(w.device)
        check(lib().rtmi_tomo_transpose_dev(self._open(), w.data_ptr(), g.data_ptr(), C.byref(st)))
        return (g, tomo_stats(st)) if stats else g

    def coverage(self):
        """A^T of a vector of ones, [qy, qx]: 0 where no ray passes -- for a mask (coverage() != 0) or a column scale"""
        return self.rmatvec(np.ones(self.info()["rows"]))

    def lsqr(self, rhs, damp=0.0, smooth=None, iter_lim=30, atol=0.0, btol=0.0, history=False, stats=False, row_weight=None,
             col_scale=None, x0=None, basis=None, smooth2=None):
        """rtmi_tomo_lsqr: min |A x - rhs|^2 + damp^2 |x|^2 + lx^2 |Dx x|^2 + ly^2 |Dy x|^2 from x = 0, smooth = (lx, ly) or None,
        every vector on the device.  -> the dict of Kirchhoff.lsqr with x [qy, qx].  row_weight [rows], col_scale and x0 [qy, qx]:
        rtmi_tomo_lsqr_weighted, min |W A D y - W (rhs - A x0)|^2 + damp^2 |y|^2 + the smoothing terms of D y, and x = x0 + D y; a
        col_scale of 0 freezes a sample at x0's value.
        basis (a TomoBasis of this handle's shape) or smooth2 = (mx2, my2), the second-difference weights: rtmi_tomo_lsqr_basis.
        With a basis the unknowns are its coefficients [my, mx]: col_scale has that shape, smooth and smooth2 act on the
        coefficient grid, x0 stays a fine model [qy, qx], and the dict gains "c" [my, mx] with x = x0 + P c."""
        rr = np.ascontiguousarray(rhs, dtype=np.float64).reshape(-1)
        if rr.size != self.info()["rows"]:
            raise ValueError(f"Tomography.lsqr: rhs must have {self.info()['rows']} values")
        iter_lim = int(iter_lim)
        if iter_lim < 1:
            raise ValueError("Tomography.lsqr: iter_lim must be >= 1")
        lp = _lib.LsqrParams()
        lp.iter_lim, lp.damp, lp.atol, lp.btol = iter_lim, float(damp), float(atol), float(btol)
        sm = None if smooth is None else np.ascontiguousarray(smooth, dtype=np.float64)
        if sm is not None and sm.shape != (2,):
            raise ValueError("Tomography.lsqr: smooth must be (lx, ly)")
        x = np.empty((self.qy, self.qx))
        hist = np.zeros((iter_lim, 4)) if history else None
        st = _lib.LsqrStats()
        c = None
        if basis is not None or smooth2 is not None:
            reg = _lib.TomoReg()
            if sm is not None:
                reg.d1[0], reg.d1[1] = sm
            if smooth2 is not None:
                s2 = np.ascontiguousarray(smooth2, dtype=np.float64)
                if s2.shape != (2,):
                    raise ValueError("Tomography.lsqr: smooth2 must be (mx2, my2)")
                reg.d2[0], reg.d2[1] = s2
            if basis is not None and not isinstance(basis, TomoBasis):
                raise TypeError("Tomography.lsqr: basis must be a TomoBasis")
            ng = self.qy * self.qx if basis is None else basis.my * basis.mx
            lo, keep = _lsqr_options("Tomography.lsqr", rr.size, ng, row_weight, col_scale, None)
            if x0 is not None:
                lo2, keep2 = _lsqr_options("Tomography.lsqr", rr.size, self.qy * self.qx, None, None, x0)
                lo.x0 = lo2.x0
            if basis is not None:
                c = np.empty((basis.my, basis.mx))
            check(lib().rtmi_tomo_lsqr_basis(self._open(), None if basis is None else basis._open(), C.byref(lp), C.byref(lo), C.byref(reg),
                                             dptr(rr), dptr(c), dptr(x), dptr(hist), C.byref(st)))
        elif row_weight is None and col_scale is None and x0 is None:
            check(lib().rtmi_tomo_lsqr(self._open(), C.byref(lp), dptr(sm), dptr(rr), dptr(x), dptr(hist), C.byref(st)))
        else:
            lo, keep = _lsqr_options("Tomography.lsqr", rr.size, self.qy * self.qx, row_weight, col_scale, x0)
            check(lib().rtmi_tomo_lsqr_weighted(self._open(), C.byref(lp), C.byref(lo), dptr(sm), dptr(rr), dptr(x), dptr(hist), C.byref(st)))
        out = {"x": x, "istop": int(st.istop), "itn": int(st.itn), "r1norm": st.r1norm, "r2norm": st.r2norm, "anorm": st.anorm,
               "arnorm": st.arnorm}
        if c is not None:
            out["c"] = c
        if history:
            out["history"] = hist[:st.itn].copy()
        if stats:
            out["stats"] = {"total_ms": st.total_ms, "operator_ms": st.operator_ms, "vector_ms": st.vector_ms,
                            "bytes_device": int(st.bytes_device)}
        return out

    # ---- many vectors at once (rtmi_tomo_*_multi): column s has the bits of the single call on column s
    def matmat(self, X, stats=False):
        """Y [S, rows] = A X[s] for X [S, qy, qx] (or [S, qy * qx]): rtmi_tomo_apply_multi in groups of at most 64 columns"""
        xx = np.ascontiguousarray(X, dtype=np.float64)
        nz = self.qy * self.qx
        if xx.ndim < 2 or xx.size != xx.shape[0] * nz:
            raise ValueError(f"Tomography.matmat: X must be [S, {self.qy}, {self.qx}] or [S, {nz}]")
        S, rows = xx.shape[0], self.info()["rows"]
        xx = xx.reshape(S, nz)
        y = np.empty((S, rows))
        st = _lib.TomoStats()
        ms = 0.0
        for a in range(0, S, _lib.LSQR_MULTI_MAX):
            b = min(S, a + _lib.LSQR_MULTI_MAX)
            check(lib().rtmi_tomo_apply_multi(self._open(), b - a, dptr(xx[a:b]), dptr(y[a:b]), C.byref(st)))
            ms += st.kernel_ms
        if stats:
            out = tomo_stats(st) if S else self.info()
            out["kernel_ms"] = ms
            return y, out
        return y

    def rmatmat(self, W, stats=False):
        """G [S, qy, qx] = A^T W[s] for W [S, rows]: rtmi_tomo_transpose_multi in groups of at most 64 columns"""
        ww = np.ascontiguousarray(W, dtype=np.float64)
        rows = self.info()["rows"]
        if ww.ndim != 2 or ww.shape[1] != rows:
            raise ValueError(f"Tomography.rmatmat: W must be [S, {rows}]")
        S = ww.shape[0]
        g = np.empty((S, self.qy, self.qx))
        st = _lib.TomoStats()
        ms, atomics = 0.0, 0
        for a in range(0, S, _lib.LSQR_MULTI_MAX):
            b = min(S, a + _lib.LSQR_MULTI_MAX)
            check(lib().rtmi_tomo_transpose_multi(self._open(), b - a, dptr(ww[a:b]), dptr(g[a:b]), C.byref(st)))
            ms += st.kernel_ms
            atomics += st.atomics
        if stats:
            out = tomo_stats(st) if S else self.info()
            out["kernel_ms"], out["atomics"] = ms, atomics
            return g, out
        return g

    def matmat_device(self, X, out=None, stats=False):
        """rtmi_tomo_apply_multi_dev on torch tensors of the handle's device: X [S, qy, qx] -> Y [S, rows] (out, if given), S <= 64"""
        import torch
        self._device_tensor("matmat_device", X, "X")
        S = int(X.shape[0]) if X.dim() >= 2 else 0
        y = torch.empty((S, self.info()["rows"]), dtype=torch.float64, device=X.device) if out is None else self._device_tensor("matmat_device", out, "out")
        st = _lib.TomoStats()
        torch.cuda.synchronize(X.device)               # the library works on the null stream
        check(lib().rtmi_tomo_apply_multi_dev(self._open(), S, X.data_ptr(), y.data_ptr(), C.byref(st)))
        return (y, tomo_stats(st)) if stats else y

    def rmatmat_device(self, W, out=None, stats=False):
        """rtmi_tomo_transpose_multi_dev on torch tensors of the handle's device: W [S, rows] -> G [S, qy, qx] (out, if given), S <= 64"""
        import torch
        self._device_tensor("rmatmat_device", W, "W")
        S = int(W.shape[0]) if W.dim() >= 2 else 0
        g = torch.empty((S, self.qy, self.qx), dtype=torch.float64, device=W.device) if out is None else self._device_tensor("rmatmat_device", out, "out")
        st = _lib.TomoStats()
        torch.cuda.synchronize(W.device)
        check(lib().rtmi_tomo_transpose_multi_dev(self._open(), S, W.data_ptr(), g.data_ptr(), C.byref(st)))
        return (g, tomo_stats(st)) if stats else g

    def lsqr_multi(self, rhs, damp=0.0, smooth=None, iter_lim=30, atol=0.0, btol=0.0, history=False, stats=False, row_weight=None,
                   col_scale=None, x0=None, basis=None, smooth2=None, group=None):
        """rtmi_tomo_lsqr_multi: Tomography.lsqr for the S right-hand sides rhs [S, rows] in lock-step -> a list of S dicts of
        Tomography.lsqr's shape, each with the bits of lsqr(rhs[s], ...).  The keyword arguments are lsqr's; col_scale and x0 are
        shared by all columns, row_weight is [rows] for all or [S, rows], one weighting per column.  Any S: the call works in
        groups of at most 64 columns, or of `group`."""
        who = "Tomography.lsqr_multi"
        rows, nz = self.info()["rows"], self.qy * self.qx
        rr = np.ascontiguousarray(rhs, dtype=np.float64)
        if rr.ndim != 2 or rr.shape[1] != rows:
            raise ValueError(f"{who}: rhs must be [S, {rows}]")
        S = rr.shape[0]
        iter_lim = int(iter_lim)
        if iter_lim < 1:
            raise ValueError(f"{who}: iter_lim must be >= 1")
        group = _lib.LSQR_MULTI_MAX if group is None else int(group)
        if not 1 <= group <= _lib.LSQR_MULTI_MAX:
            raise ValueError(f"{who}: group must be in 1 .. {_lib.LSQR_MULTI_MAX}")
        lp = _lib.LsqrParams()
        lp.iter_lim, lp.damp, lp.atol, lp.btol = iter_lim, float(damp), float(atol), float(btol)
        reg = _lib.TomoReg()
        for name, pair, dst in (("smooth", smooth, reg.d1), ("smooth2", smooth2, reg.d2)):
            if pair is not None:
                pp = np.ascontiguousarray(pair, dtype=np.float64)
                if pp.shape != (2,):
                    raise ValueError(f"{who}: {name} must be a pair")
                dst[0], dst[1] = pp
        if basis is not None and not isinstance(basis, TomoBasis):
            raise TypeError(f"{who}: basis must be a TomoBasis")
        gshape = (self.qy, self.qx) if basis is None else (basis.my, basis.mx)
        lo, keep = _lsqr_options(who, rows, gshape[0] * gshape[1], None, col_scale, None)
        if x0 is not None:
            lo2, keep2 = _lsqr_options(who, rows, nz, None, None, x0)
            lo.x0 = lo2.x0
        wr, flags = None, 0
        if row_weight is not None:
            wr = np.ascontiguousarray(row_weight, dtype=np.float64)
            if wr.shape == (S, rows) and wr.ndim == 2:
                flags = _lib.LSQR_MULTI_ROW_WEIGHT
            elif wr.size == rows and wr.ndim <= 1 or wr.shape == (1, rows):
                wr = wr.reshape(rows)
            else:
                raise ValueError(f"{who}: row_weight must be [{rows}] or [S, {rows}]")
        out = []
        for a in range(0, S, group):
            b = min(S, a + group)
            n = b - a
            x = np.empty((n, self.qy, self.qx))
            c = np.empty((n,) + gshape) if basis is not None else None
            hist = np.zeros((n, iter_lim, 4)) if history else None
            st = (_lib.LsqrStats * n)()
            if wr is not None:
                wg = np.ascontiguousarray(wr[a:b]) if flags else wr
                lo.row_weight = dptr(wg)
            check(lib().rtmi_tomo_lsqr_multi(self._open(), None if basis is None else basis._open(), C.byref(lp), C.byref(lo), C.byref(reg),
                                             n, flags, dptr(np.ascontiguousarray(rr[a:b])), dptr(c), dptr(x), dptr(hist), st))
            for s in range(n):
                o = {"x": x[s], "istop": int(st[s].istop), "itn": int(st[s].itn), "r1norm": st[s].r1norm, "r2norm": st[s].r2norm,
                     "anorm": st[s].anorm, "arnorm": st[s].arnorm}
                if c is not None:
                    o["c"] = c[s]
                if history:
                    o["history"] = hist[s, :st[s].itn].copy()
                if stats:
                    o["stats"] = {"total_ms": st[s].total_ms, "operator_ms": st[s].operator_ms, "vector_ms": st[s].vector_ms,
                                  "bytes_device": int(st[s].bytes_device)}
                out.append(o)
        return out

    def recover(self, models, **lsqr_kw):
        """The resolution test: d_s = A m_s (matmat), then lsqr_multi(d, **lsqr_kw) -> (the recovered models [S, qy, qx], the
        dicts).  models [S, qy, qx], e.g. checkerboard(...) or spikes(...) stacked."""
        mm = np.ascontiguousarray(models, dtype=np.float64)
        if mm.ndim != 3 or mm.shape[1:] != (self.qy, self.qx):
            raise ValueError(f"Tomography.recover: models must be [S, {self.qy}, {self.qx}]")
        outs = self.lsqr_multi(self.matmat(mm), **lsqr_kw)
        return np.stack([o["x"] for o in outs]) if outs else np.empty((0, self.qy, self.qx)), outs

    def bootstrap(self, rhs, n, seed, results=False, **lsqr_kw):
        """n bootstrap replicates of lsqr(rhs, ...): replicate k weighs row r by the square root of its multiplicity in a draw of
        `rows` rows with replacement (bootstrap_weights(rows, n, seed)), times the caller's row_weight [rows], if given; one
        lsqr_multi over them.  -> (mean, standard deviation with ddof 1) of x over the replicates, [qy, qx] each, and with
        results=True the per-replicate dicts as well."""
        rows = self.info()["rows"]
        rr = np.ascontiguousarray(rhs, dtype=np.float64).reshape(-1)
        if rr.size != rows:
            raise ValueError(f"Tomography.bootstrap: rhs must have {rows} values")
        w = bootstrap_weights(rows, n, seed)
        base = lsqr_kw.pop("row_weight", None)
        if base is not None:
            bb = np.ascontiguousarray(base, dtype=np.float64).reshape(-1)
            if bb.size != rows:
                raise ValueError(f"Tomography.bootstrap: row_weight must have {rows} values")
            w = w * bb[None, :]
        outs = self.lsqr_multi(np.broadcast_to(rr, (len(w), rows)), row_weight=w, **lsqr_kw)
        xs = np.stack([o["x"] for o in outs])
        mean, std = xs.mean(axis=0), xs.std(axis=0, ddof=1)
        return (mean, std, outs) if results else (mean, std)

    def read(self):
        """rtmi_tomo_read: (row_ptr [rows + 1], base [segments], val [segments, 4]), rows in order, segments in visit order"""
        i = self.info()
        row_ptr = np.zeros(i["rows"] + 1, dtype=np.int64)
        base = np.empty(i["segments"], dtype=np.int32)
        val = np.empty((i["segments"], 4))
        check(lib().rtmi_tomo_read(self._open(), row_ptr.ctypes.data_as(C.POINTER(C.c_int64)), base.ctypes.data_as(_lib._ip), dptr(val)))
        return row_ptr, base, val

    def to_csr(self):
        """The matrix as scipy.sparse CSR [rows, qy * qx]; segments of a row that share a column are summed"""
        import scipy.sparse as sp
        row_ptr, base, val = self.read()
        rows = len(row_ptr) - 1
        r = np.repeat(np.arange(rows), np.diff(row_ptr))
        b = base.astype(np.int64)
        cols = np.stack([b, b + 1, b + self.qx, b + self.qx + 1], axis=1)
        return sp.coo_matrix((val.ravel(), (np.repeat(r, 4), cols.ravel())), shape=(rows, self.qy * self.qx)).tocsr()

    def as_linear_operator(self):
        from scipy.sparse.linalg import LinearOperator
        return LinearOperator(self.shape, matvec=lambda x: self.matvec(x), rmatvec=lambda w: self.rmatvec(w).reshape(-1), dtype=np.float64)

    def close(self):
        if self._h:
            lib().rtmi_tomo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def checkerboard(qy, qx, cell, amplitude=1.0):
    """A checkerboard model [qy, qx] for Tomography.recover: squares of `cell` samples (or cell = (cy, cx)), +amplitude where
    (i // cy + j // cx) is even -- the square at the origin --, -amplitude where it is odd.  Pure numpy."""
    cy, cx = (int(cell), int(cell)) if np.ndim(cell) == 0 else (int(cell[0]), int(cell[1]))
    if cy < 1 or cx < 1:
        raise ValueError("checkerboard: cell must be >= 1")
    odd = (np.arange(int(qy))[:, None] // cy + np.arange(int(qx))[None, :] // cx) % 2 == 1
    return np.where(odd, -float(amplitude), float(amplitude))


def spikes(qy, qx, nodes, amplitude=1.0):
    """One spike model per node for Tomography.recover: [len(nodes), qy, qx], model s is `amplitude` at nodes[s] = (i, j) and
    0.0 elsewhere.  Pure numpy."""
    nn = np.asarray(nodes, dtype=np.int64).reshape(-1, 2)
    if len(nn) and (nn.min() < 0 or nn[:, 0].max() >= qy or nn[:, 1].max() >= qx):
        raise ValueError("spikes: a node lies outside the grid")
    out = np.zeros((len(nn), int(qy), int(qx)))
    out[np.arange(len(nn)), nn[:, 0], nn[:, 1]] = float(amplitude)
    return out


def bootstrap_weights(rows, n, seed):
    """Row weights [n, rows] of n bootstrap replicates: replicate k draws `rows` row indices with replacement from
    numpy.random.Generator(numpy.random.PCG64(seed)), the replicates one after the other from the one generator; a row's weight is
    the square root of its multiplicity in the draw, 0.0 for a row not drawn, so that the weighted misfit counts a row as often
    as it was drawn and every replicate's squared weights sum to `rows`.  Pure numpy."""
    rows, n = int(rows), int(n)
    if rows < 1 or n < 1:
        raise ValueError("bootstrap_weights: rows and n must be >= 1")
    rng = np.random.Generator(np.random.PCG64(seed))
    w = np.empty((n, rows))
    for k in range(n):
        w[k] = np.sqrt(np.bincount(rng.integers(0, rows, size=rows), minlength=rows).astype(np.float64))
    return w


def bspline_axis(q, m, degree):
    """rtmi_bspline_axis: (first [q] int32, wgt [q, degree + 1]) of uniform B-splines of degree 0, 1 or 3 from m coefficients onto
    q samples, the first and last sample on the ends of the knot span (include/rtmi.h).  Host only: no device is touched."""
    q, m, degree = int(q), int(m), int(degree)
    first = np.zeros(max(q, 1), dtype=np.int32)
    wgt = np.zeros((max(q, 1), max(degree, 0) + 1))
    check(lib().rtmi_bspline_axis(q, m, degree, first.ctypes.data_as(_lib._ip), dptr(wgt)))
    return first, wgt


class TomoBasis:
    """A separable model basis P = Py (x) Px for a Tomography handle (rtmi_tomo_basis_*): coefficients c [my, mx] -> samples
    x [qy, qx].  An axis is (first [q] int32, wgt [q, B]), B in 1 .. 4: sample j carries wgt[j, b] on coefficient first[j] + b;
    first is non-decreasing.  prolong is P, restrict its transpose entry for entry; Tomography.lsqr(basis=...) solves for c.
    The basis copies what it needs from the handle and may outlive it.  shape = (qy * qx, my * mx)."""

    def __init__(self, tomo, first_x, wgt_x, first_y, wgt_y, mx, my):
        self._h = None
        self.qx, self.qy, self.mx, self.my = tomo.qx, tomo.qy, int(mx), int(my)
        fx = np.ascontiguousarray(first_x, dtype=np.int32).reshape(-1)
        fy = np.ascontiguousarray(first_y, dtype=np.int32).reshape(-1)
        wx = np.ascontiguousarray(wgt_x, dtype=np.float64).reshape(len(fx), -1)
        wy = np.ascontiguousarray(wgt_y, dtype=np.float64).reshape(len(fy), -1)
        if len(fx) != self.qx or len(fy) != self.qy:
            raise ValueError(f"TomoBasis: first_x and first_y must have {self.qx} and {self.qy} values, the handle's qx and qy")
        h = C.c_void_p()
        check(lib().rtmi_tomo_basis_create(tomo._open(), self.mx, wx.shape[1], fx.ctypes.data_as(_lib._ip), dptr(wx), self.my, wy.shape[1],
                                           fy.ctypes.data_as(_lib._ip), dptr(wy), C.byref(h)))
        self._h = h

    @classmethod
    def bspline(cls, tomo, mx, my, degree=3):
        """Uniform B-splines (bspline_axis) of `degree` on both axes, or of (dx, dy)"""
        dx, dy = (degree, degree) if np.ndim(degree) == 0 else degree
        fx, wx = bspline_axis(tomo.qx, mx, dx)
        fy, wy = bspline_axis(tomo.qy, my, dy)
        return cls(tomo, fx, wx, fy, wy, mx, my)

    def _open(self):
        if not self._h:
            raise ValueError("TomoBasis: the handle is closed")
        return self._h

    @property
    def shape(self):
        return (self.qy * self.qx, self.my * self.mx)

    def prolong(self, c):
        """x [qy, qx] = P c for c [my, mx] (or flat)"""
        cc = np.ascontiguousarray(c, dtype=np.float64)
        if cc.size != self.my * self.mx:
            raise ValueError(f"TomoBasis.prolong: c must have {self.my * self.mx} values")
        x = np.empty((self.qy, self.qx))
        check(lib().rtmi_tomo_basis_prolong(self._open(), dptr(cc), dptr(x)))
        return x

    def restrict(self, x):
        """g [my, mx] = P^T x for x [qy, qx] (or flat): one fixed summation order, the same bits under every launch shape"""
        xx = np.ascontiguousarray(x, dtype=np.float64)
        if xx.size != self.qy * self.qx:
            raise ValueError(f"TomoBasis.restrict: x must have {self.qy * self.qx} values")
        g = np.empty((self.my, self.mx))
        check(lib().rtmi_tomo_basis_restrict(self._open(), dptr(xx), dptr(g)))
        return g

    _device_tensor = Tomography._device_tensor

    def prolong_device(self, c, out=None):
        """rtmi_tomo_basis_prolong_dev on torch tensors of the basis's device: c [my, mx] -> x [qy, qx] (out, if given)"""
        import torch
        self._device_tensor("prolong_device", c, "c")
        x = torch.empty((self.qy, self.qx), dtype=torch.float64, device=c.device) if out is None else self._device_tensor("prolong_device", out, "out")
        torch.cuda.synchronize(c.device)               # the library works on the null stream
        check(lib().rtmi_tomo_basis_prolong_dev(self._open(), c.data_ptr(), x.data_ptr()))
        return x

    def restrict_device(self, x, out=None):
        """rtmi_tomo_basis_restrict_dev on torch tensors of the basis's device: x [qy, qx] -> g [my, mx] (out, if given)"""
        import torch
        self._device_tensor("restrict_device", x, "x")
        g = torch.empty((self.my, self.mx), dtype=torch.float64, device=x.device) if out is None else self._device_tensor("restrict_device", out, "out")
        torch.cuda.synchronize(x.device)
        check(lib().rtmi_tomo_basis_restrict_dev(self._open(), x.data_ptr(), g.data_ptr()))
        return g

    def close(self):
        if self._h:
            lib().rtmi_tomo_basis_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _two_point_paraxial(field, p, sx, sy, line, arr, kmax):
    """The paraxial columns of two_point's converged arrivals, by public calls only: one fresh batch of the
    converged (source, launch angle) rays with the solver's parameters -- sized by a count pass without a record, as
    rtmi_two_point sizes its own --, its crossings and its paraxial quantities at them; each arrival takes the crossing whose
    u and T are bit-equal to its own (rtmi_two_point's promise: its arrivals are exactly what rtmi_crossings gives on such a
    fresh batch)."""
    keys = ("Q2", "P2", "J", "G", "kmah")
    res = {k: np.full(arr["T"].shape, np.nan) for k in keys}
    idx = np.argwhere(arr["status"] == _lib.ARRIVAL_CONVERGED)
    if len(idx) == 0:
        return res
    R = len(idx)
    x0 = np.ascontiguousarray(sx[idx[:, 0]]); y0 = np.ascontiguousarray(sy[idx[:, 0]])
    th = np.ascontiguousarray(arr["theta0"][tuple(idx.T)])
    q = Params.from_buffer_copy(p)
    q.sort_rays = 0; q.no_n_ray = 1; q.lazy_clear = 0; q.ext_s_ray = None; q.ext_n_ray = None

    def batch(stride, rows):
        q.record_stride = stride; q.rec_rows = rows
        h = C.c_void_p()
        check(lib().rtmi_batch_create(field._h, C.byref(q), R, dptr(x0), dptr(y0), dptr(th), None, C.byref(h)))
        return h
    h = batch(0, 0)
    try:
        check(lib().rtmi_run(h))
        d = np.empty((3, R))
        check(lib().rtmi_read_d_ray(h, dptr(d)))
    finally:
        lib().rtmi_batch_destroy(h)
    h = batch(1, int(d[2].max()) + 1)
    try:
        check(lib().rtmi_run(h))
        cnt = np.empty(R, dtype=np.int32)
        cr = np.empty((kmax, len(CROSSING_FIELDS), R))
        check(lib().rtmi_crossings(h, dptr(line), kmax, cnt.ctypes.data_as(_lib._ip), dptr(cr)))
        pc = np.empty(R, dtype=np.int32)
        at = np.empty((kmax, len(PARAXIAL_FIELDS), R))
        end = np.empty((len(PARAXIAL_FIELDS), R))
        check(lib().rtmi_paraxial(h, dptr(line), kmax, pc.ctypes.data_as(_lib._ip), dptr(at), dptr(end)))
    finally:
        lib().rtmi_batch_destroy(h)
    iu, iT = CROSSING_FIELDS.index("u"), CROSSING_FIELDS.index("T")
    for r, (s_, j, a) in enumerate(idx):
        hit = np.nonzero((cr[:, iu, r] == arr["u"][s_, j, a]) & (cr[:, iT, r] == arr["T"][s_, j, a]))[0]
        if len(hit) == 0:
            raise RuntimeError(f"two_point: no crossing of the re-traced ray matches arrival {(s_, j, a)}")
        for k in keys:
            res[k][s_, j, a] = at[hit[0], PARAXIAL_FIELDS.index(k), r]
    return res


GRID_FIELDS = ("T", "theta0", "theta", "ray", "step")                            # rtmi_first_arrival_grid's out columns
GRID_AMPLITUDE_FIELDS = ("J", "G", "kmah")                                       # ... and with amplitude


def grid_params(grid, max_gap=None, max_dtheta=None, amplitude=False):
    """rtmi_grid_params of grid = (gx0, gdx, nx, gy0, gdy, ny); None / 0 take the library's defaults"""
    gx0, gdx, nx, gy0, gdy, ny = grid
    gp = _lib.GridParams()
    gp.gx0 = float(gx0); gp.gdx = float(gdx); gp.nx = int(nx)
    gp.gy0 = float(gy0); gp.gdy = float(gdy); gp.ny = int(ny)
    gp.max_gap = float(max_gap or 0.0); gp.max_dtheta = float(max_dtheta or 0.0)
    gp.amplitude = int(bool(amplitude))
    return gp


def _grid_call(call, S, grid, max_gap, max_dtheta, amplitude, stats):
    gp = grid_params(grid, max_gap, max_dtheta, amplitude)
    names = GRID_FIELDS + (GRID_AMPLITUDE_FIELDS if amplitude else ())
    nx, ny = max(int(gp.nx), 0), max(int(gp.ny), 0)
    count = np.zeros((max(S, 0), ny, nx), dtype=np.int32)
    out = np.empty((max(S, 0), len(names), ny, nx))
    st = _lib.GridStats()
    check(call(C.byref(gp), count.ctypes.data_as(_lib._ip), dptr(out), C.byref(st)))
    d = {"count": count}
    for q, k in enumerate(names):
        d[k] = out[:, q].copy()
    if stats:
        d["stats"] = grid_stats(st)
    return d


def grid_stats(st):
    return {"cells": st.cells, "skipped_cells": st.skipped_cells, "triangles": st.triangles, "folded": st.folded,
            "atomics": [int(v) for v in st.atomics], "pass_ms": [float(v) for v in st.pass_ms], "max_gap": st.max_gap,
            "max_dtheta": st.max_dtheta}


def debug_grid_rows(x, y, T, theta, last, theta0, grid, fan_size=None, max_gap=None, max_dtheta=None, stats=False):
    """rtmi_first_arrival_grid's kernels on caller-supplied rows (rtmi_debug_grid_rows): x, y, T, theta [rows, R], last [R],
    theta0 [R].  Returns what Batch.first_arrival_grid returns (no amplitude)."""
    x, y, T, th = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, T, theta))
    rows, R = x.shape
    assert y.shape == T.shape == th.shape == (rows, R)
    la = np.ascontiguousarray(last, dtype=np.int32)
    t0 = np.ascontiguousarray(theta0, dtype=np.float64)
    assert la.shape == t0.shape == (R,)
    M = R if fan_size is None else int(fan_size)
    return _grid_call(lambda gp, cnt, out, st: lib().rtmi_debug_grid_rows(rows, R, M, dptr(x), dptr(y), dptr(T), dptr(th),
                                                                          la.ctypes.data_as(_lib._ip), dptr(t0), gp, cnt, out, st),
                      R // M if M >= 1 else 0, grid, max_gap, max_dtheta, False, stats)


def arrival_params(arrivals=1, order="time"):
    """rtmi_arrival_params: order "time" or "amplitude" (or the constant itself)"""
    ap = _lib.ArrivalParams()
    ap.karr = int(arrivals)
    ap.order = _lib.ARRIVAL_ORDERS[order] if isinstance(order, str) else int(order)
    return ap


def _arrival_call(call, S, grid, arrivals, order, max_gap, max_dtheta, amplitude, stats, count_only=False):
    gp = grid_params(grid, max_gap, max_dtheta, amplitude)
    ap = arrival_params(arrivals, order)
    names = GRID_FIELDS + (GRID_AMPLITUDE_FIELDS if amplitude else ())
    nx, ny, K = max(int(gp.nx), 0), max(int(gp.ny), 0), min(max(int(ap.karr), 0), _lib.MAX_ARRIVALS)
    count = np.zeros((max(S, 0), ny, nx), dtype=np.int32)
    out = None if count_only else np.empty((max(S, 0), K, len(names), ny, nx))
    st = _lib.ArrivalStats()
    check(call(C.byref(gp), C.byref(ap), count.ctypes.data_as(_lib._ip), dptr(out), C.byref(st)))
    d = {"count": count}
    if out is not None:
        for q, k in enumerate(names):
            d[k] = out[:, :, q].copy()
    if stats:
        d["stats"] = dict(grid_stats(st), candidates=int(st.candidates), scan_ms=float(st.scan_ms))
    return d


def debug_arrival_rows(x, y, T, theta, last, theta0, grid, arrivals=1, order="time", J=None, kmah=None, n=None, fan_size=None,
                       max_gap=None, max_dtheta=None, amplitude=False, stats=False):
    """rtmi_arrival_grid's kernels on caller-supplied rows (rtmi_debug_arrival_rows): x, y, T, theta [rows, R], last [R],
    theta0 [R]; J, kmah, n [rows, R] for the amplitude columns and for order "amplitude".  Returns what Batch.arrival_grid returns."""
    x, y, T, th = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, T, theta))
    rows, R = x.shape
    assert y.shape == T.shape == th.shape == (rows, R)
    la = np.ascontiguousarray(last, dtype=np.int32)
    t0 = np.ascontiguousarray(theta0, dtype=np.float64)
    assert la.shape == t0.shape == (R,)
    Ja, na = (None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (J, n))
    ka = None if kmah is None else np.ascontiguousarray(kmah, dtype=np.int32)
    assert all(a is None or a.shape == (rows, R) for a in (Ja, ka, na))
    M = R if fan_size is None else int(fan_size)
    ip = _lib._ip
    return _arrival_call(lambda gp, ap, cnt, out, st: lib().rtmi_debug_arrival_rows(
        rows, R, M, dptr(x), dptr(y), dptr(T), dptr(th), la.ctypes.data_as(ip), dptr(t0), dptr(Ja),
        None if ka is None else ka.ctypes.data_as(ip), dptr(na), gp, ap, cnt, out, st),
        R // M if M >= 1 else 0, grid, arrivals, order, max_gap, max_dtheta, amplitude, stats)


def traveltime_table(selected_func, field, sources, grid, *, thetas, step, max_size, box, gamma=1, amplitude=False, mem_budget=0,
                     max_gap=None, max_dtheta=None, stats=False, arrivals=None, order="time", fill=None, fill_attributes=False,
                     fill_scheme="plain", **batch_kw):
    """First-arrival tables from many sources onto one grid, by public calls only: a fan of launch angles
    `thetas` per source (sources: (S, 2) array of (x, y)).  1. A count pass without a record sizes rec_rows to the longest ray.
    2. Sources are grouped so that each group's record (48 bytes per row and ray in fp64, 24 in fp32; 12 more with amplitude,
    for the per-row J and kmah) stays under mem_budget (default 8 GiB).  3. One batch per group is traced and its grid taken
    (Batch.first_arrival_grid).  Each source's table depends on its own rays only, so the grouping changes no bit.  batch_kw go
    to Batch (launch_mode, sort_rays, reference_order, ...).  Returns a dict of [S, ny, nx] arrays as first_arrival_grid; with
    stats=True also 'stats' (rec_rows, groups, count_ms, trace_ms, grid_ms: host wall times, and the grid calls' summed
    counters).  arrivals=K (with order "time" or "amplitude") takes Batch.arrival_grid instead: arrays of [S, K, ny, nx], count
    [S, ny, nx]; a group's candidate list (16 bytes per candidate, counted by a count-only call before it is allocated) then
    counts against mem_budget too, and a group over it is traced again in halves.  fill="eikonal" completes T after the ray-cell
    pass (eikonal_fill with its defaults): every node the covered ones or the source can reach gets a first
    arrival, with arrivals=K in slot 0 only, and 'filled' [S, ny, nx] (uint8) marks those nodes; count and the other columns
    stay as they are, 0 and NaN there, since no ray reaches them.  fill=None is the ray-cell result alone.  With
    fill_attributes=True (it needs fill="eikonal") the filled nodes also get theta0 and theta, and with amplitude=True J and G,
    carried from the covered nodes through the fill's network (eikonal_attributes), and kmah 0; with arrivals=K in
    slot 0 only.  ray, step and count stay as they are.  fill_scheme "plain" or "factored" is eikonal_fill's scheme (DESIGN.md
    39); covered nodes keep their bits under either."""
    if fill not in (None, "eikonal"):
        raise ValueError('traveltime_table: fill must be None or "eikonal"')
    if fill_scheme not in _lib.EIKONAL_SCHEMES:
        raise ValueError('traveltime_table: fill_scheme must be "plain" or "factored"')
    if fill_attributes and fill is None:
        raise ValueError('traveltime_table: fill_attributes needs fill="eikonal"')
    src = np.asarray(sources, dtype=np.float64).reshape(-1, 2)
    th = np.ascontiguousarray(thetas, dtype=np.float64)
    S, M = len(src), len(th)
    batch_kw = dict(batch_kw)
    batch_kw.pop("keep_n_ray", None)
    t0 = time.perf_counter()
    c = Batch(field, selected_func, step, max_size, box, gamma, np.tile(th, S), np.repeat(src[:, 0], M), np.repeat(src[:, 1], M),
              record_stride=0, keep_n_ray=False, **batch_kw)
    try:
        c.run()
        rows = int(c.d_ray()[2].max()) + 1
    finally:
        c.close()
    t1 = time.perf_counter()
    by_amp = arrivals is not None and _lib.ARRIVAL_ORDERS.get(order, order) == _lib.ARRIVAL_BY_AMPLITUDE
    per_ray = rows * ((48 if field.dtype == F64 else 24) + (12 if amplitude or by_amp else 0))
    budget = int(mem_budget) if mem_budget else 8 << 30
    G = max(1, min(S, budget // max(per_ray * M, 1)))
    res, tot = None, {"rec_rows": rows, "groups": 0, "count_ms": (t1 - t0) * 1e3, "trace_ms": 0.0, "grid_ms": 0.0}
    g0 = 0
    while g0 < S:
        sg = src[g0:g0 + G]
        ta = time.perf_counter()
        b = Batch(field, selected_func, step, max_size, box, gamma, np.tile(th, len(sg)), np.repeat(sg[:, 0], M),
                  np.repeat(sg[:, 1], M), record_stride=1, rec_rows=rows, keep_n_ray=False, **batch_kw)
        try:
            b.run()
            b.sync()
            tb = time.perf_counter()
            gkw = dict(fan_size=M, max_gap=max_gap, max_dtheta=max_dtheta, amplitude=amplitude, stats=True)
            if arrivals is None:
                r = b.first_arrival_grid(grid, **gkw)
            else:
                gkw.update(arrivals=arrivals, order=order)
                listed = 16 * b.arrival_grid(grid, count_only=True, **gkw)["stats"]["candidates"]
                fits = len(sg) == 1 or per_ray * M * len(sg) + listed <= budget
                r = b.arrival_grid(grid, **gkw) if fits else None
        finally:
            b.close()
        if r is None:                           # the candidate list would not fit beside the record: a smaller group
            G = max(1, len(sg) // 2)
            continue
        tc = time.perf_counter()
        tot["groups"] += 1
        tot["trace_ms"] += (tb - ta) * 1e3
        tot["grid_ms"] += (tc - tb) * 1e3
        st = r.pop("stats")
        for k in ("cells", "skipped_cells", "triangles", "folded"):
            tot[k] = tot.get(k, 0) + st[k]
        tot["atomics"] = [a + b_ for a, b_ in zip(tot.get("atomics", [0, 0, 0]), st["atomics"])]
        tot["pass_ms"] = [a + b_ for a, b_ in zip(tot.get("pass_ms", [0.0] * 3), st["pass_ms"])]
        if arrivals is not None:
            tot["candidates"] = tot.get("candidates", 0) + st["candidates"]
        if res is None:
            res = {k: np.empty((S,) + v.shape[1:], dtype=v.dtype) for k, v in r.items()}
        for k, v in r.items():
            res[k][g0:g0 + len(sg)] = v
        g0 += len(sg)
    if fill is not None:
        T0 = np.ascontiguousarray(res["T"][:, 0] if arrivals is not None else res["T"])
        done = eikonal_fill(field, src, grid, T0, stats=True, scheme=fill_scheme)
        if arrivals is not None:
            res["T"][:, 0] = done["T"]
        else:
            res["T"] = done["T"]
        res["filled"] = done["filled"]
        tot["eikonal"] = done["stats"]
        if fill_attributes:
            slot = (lambda a: a[:, 0]) if arrivals is not None else (lambda a: a)
            names = ("theta0", "theta") + (("J", "G") if amplitude else ())
            att = eikonal_attributes(field, src, grid, done["T"], done["filled"], stats=True,
                                     **{k: np.ascontiguousarray(slot(res[k])) for k in names})
            for k in names:
                slot(res[k])[...] = att[k]
            if amplitude and "kmah" in res:
                slot(res["kmah"])[done["filled"] != 0] = 0
            tot["eikonal_attributes"] = att["stats"]
    if stats:
        res["stats"] = tot
    return res


def eikonal_params(grid, ball=2.0, max_rounds=0, _global_path=False, _width=0, scheme="plain", linearise="plain"):
    """rtmi_eikonal_params of grid = (gx0, gdx, nx, gy0, gdy, ny); scheme "plain" or "factored" is the fills'; linearise "plain" or
    "factored" is the tangent's and the adjoint's, and "factored" goes with the factored fill alone: scheme is then
    RTMI_EIKONAL_FACTORED_LIN; _global_path and _width (the chunk width of the batched sweeps) are for tests: no result depends on
    them"""
    gx0, gdx, nx, gy0, gdy, ny = grid
    if scheme not in _lib.EIKONAL_SCHEMES:
        raise ValueError('eikonal: scheme must be "plain" or "factored"')
    if not isinstance(linearise, str) or linearise not in _lib.EIKONAL_LINEARISE:
        raise ValueError('eikonal: linearise must be "plain" or "factored"')
    ep = _lib.EikonalParams()
    ep.gx0 = float(gx0); ep.gdx = float(gdx); ep.nx = int(nx)
    ep.gy0 = float(gy0); ep.gdy = float(gdy); ep.ny = int(ny)
    ep.ball = float(ball); ep.max_rounds = int(max_rounds); ep.scheme = _lib.EIKONAL_SCHEMES[scheme]
    if linearise == "factored":
        ep.scheme = _lib.EIKONAL_FACTORED_LIN
    ep.reserved[0] = int(bool(_global_path))
    ep.reserved[1] = int(_width)
    return ep


def eikonal_stats(st):
    return {"free_nodes": int(st.free_nodes), "filled": int(st.filled), "unreached": int(st.unreached), "changes": int(st.changes),
            "rounds_max": int(st.rounds_max), "path": _lib.EIKONAL_PATHS.get(st.path, st.path), "kernel_ms": st.kernel_ms}


def _eikonal_medium(who, field_or_n, src, grid, n_src):
    """n [ny, nx] at the nodes and n_src [S] at the sources: a Field is sampled with Field.n_gradient, an array is n itself"""
    gx0, gdx, nx, gy0, gdy, ny = grid
    if isinstance(field_or_n, Field):
        X, Y = np.meshgrid(float(gx0) + np.arange(int(nx)) * float(gdx), float(gy0) + np.arange(int(ny)) * float(gdy))
        n = field_or_n.n_gradient(X.reshape(-1), Y.reshape(-1))[0].reshape(int(ny), int(nx))
        if n_src is None and len(src):
            n_src = field_or_n.n_gradient(src[:, 0], src[:, 1])[0]
    else:
        n = field_or_n
        if n_src is None and len(src):
            raise ValueError(f"{who}: an array for n needs n_src=, the slowness at each source")
    return n, (np.zeros(0) if n_src is None else n_src)


def eikonal_fill(field_or_n, sources, grid, T=None, *, n_src=None, ball=2.0, max_rounds=0, stats=False, scheme="plain",
                 _global_path=False):
    """Complete traveltime tables by a first-arrival eikonal solve on the device (rtmi_eikonal_fill, include/rtmi.h; DESIGN.md
    34): the first-order Godunov upwind scheme for |grad T| = n by fast sweeping, seeded by the finite nodes of T and an analytic
    ball of `ball` cells round each source (negative: none).  field_or_n: a Field, sampled at the nodes and at the sources, or
    n [ny, nx] with n_src [S].  sources [S, 2]; grid = (gx0, gdx, nx, gy0, gdy, ny); T [S, ny, nx] (not modified), or None: all
    NaN, a point-source solve without rays.  Nodes where n is not finite or <= 0 are obstacles.  Returns a dict:
      T [S, ny, nx]      finite inputs keep their bits; every other node that the seeds can reach has its first arrival; NaN
                         where none can (and an obstacle keeps its input)
      filled             [S, ny, nx] uint8, 1 where the call gave the value
      rounds, converged  [S]: the rounds of four sweeps that ran (at most max_rounds, 0: 64), and whether the last changed nothing
    and with stats=True 'stats'.  The error is first order in the spacing: about 1 % of the largest T where the ball is the
    only seed, 1e-3 to 1e-4 in a shadow of a table that rays cover elsewhere -- shoot the full fan and let this fill the rest.
    scheme="factored"  differences T - n_src r in place of T: still first order, but 6 to 10 times less error
    where the ball is the only seed, exact to rounding in a constant medium, at the price of some ten rounds in place of two; far
    from the source, in the shadow of a table, it gains nothing.  The default "plain" keeps every bit."""
    who = "eikonal_fill"
    src = np.ascontiguousarray(np.asarray(sources, dtype=np.float64).reshape(-1, 2))
    S, nx, ny = len(src), int(grid[2]), int(grid[5])
    n, n_src = _eikonal_medium(who, field_or_n, src, grid, n_src)
    n = np.ascontiguousarray(n, dtype=np.float64)
    ns = np.ascontiguousarray(n_src, dtype=np.float64).reshape(-1)
    if nx >= 1 and ny >= 1 and n.shape != (ny, nx):
        raise ValueError(f"{who}: n must be [ny, nx] of the grid")
    if len(ns) != S:
        raise ValueError(f"{who}: n_src must be [S]")
    shape = (S, max(ny, 0), max(nx, 0))
    if T is None:
        out = np.full(shape, np.nan)
    else:
        out = np.array(T, dtype=np.float64, order="C")
        if out.shape != shape:
            raise ValueError(f"{who}: T must be [S, ny, nx]")
    rounds = np.zeros((S, 2), dtype=np.int32)
    filled = np.zeros(shape, dtype=np.uint8)
    ep = eikonal_params(grid, ball, max_rounds, _global_path, scheme=scheme)
    st = _lib.EikonalStats()
    check(lib().rtmi_eikonal_fill(C.byref(ep), dptr(n), S, dptr(src), dptr(ns), dptr(out), rounds.ctypes.data_as(_lib._ip),
                                  filled.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(st)))
    res = {"T": out, "rounds": rounds[:, 0].copy(), "converged": rounds[:, 1].copy(), "filled": filled}
    if stats:
        res["stats"] = eikonal_stats(st)
    return res


def eikonal_fill_device(field_or_n, sources, grid, T=None, *, n_src=None, ball=2.0, max_rounds=0, stats=False, scheme="plain",
                        _global_path=False):
    """eikonal_fill on torch tensors of one GPU, with no host copy of the tables (rtmi_eikonal_fill_dev): n [ny, nx], sources
    [S, 2], n_src [S] and T [S, ny, nx] in fp64, contiguous; a Field in place of n is sampled as in eikonal_fill.  T is
    completed IN PLACE and returned; None: a new table from an all-NaN input.  filled is a uint8 tensor on the device; rounds
    and converged are numpy arrays.  The same bits."""
    import torch
    who = "eikonal_fill_device"
    n = field_or_n
    if isinstance(field_or_n, Field):
        if not isinstance(sources, torch.Tensor):
            raise TypeError(f"{who}: sources must be a torch tensor")
        hn, hs = _eikonal_medium(who, field_or_n, sources.detach().cpu().numpy().reshape(-1, 2), grid,
                                 None if n_src is None else n_src.detach().cpu().numpy())
        n = torch.as_tensor(np.ascontiguousarray(hn), device=sources.device)
        n_src = torch.as_tensor(np.ascontiguousarray(hs, dtype=np.float64), device=sources.device)
    elif n_src is None:
        raise ValueError(f"{who}: a tensor for n needs n_src=, the slowness at each source")
    for name, a in (("n", n), ("sources", sources), ("n_src", n_src), ("T", T)):
        if a is None and name == "T":
            continue
        if not isinstance(a, torch.Tensor):
            raise TypeError(f"{who}: {name} must be a torch tensor")
        if a.dtype != torch.float64:
            raise TypeError(f"{who}: {name} must be torch.float64")
        if not a.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous")
        if not a.is_cuda:
            raise ValueError(f"{who}: {name} must be a tensor on a GPU, not on the host")
    nx, ny = int(grid[2]), int(grid[5])
    if sources.dim() != 2 or sources.shape[1] != 2:
        raise ValueError(f"{who}: sources must be [S, 2]")
    S = sources.shape[0]
    if tuple(n.shape) != (ny, nx):
        raise ValueError(f"{who}: n must be [ny, nx] of the grid")
    if tuple(n_src.shape) != (S,):
        raise ValueError(f"{who}: n_src must be [S]")
    if T is None:
        T = torch.full((S, ny, nx), float("nan"), dtype=torch.float64, device=n.device)
    elif tuple(T.shape) != (S, ny, nx):
        raise ValueError(f"{who}: T must be [S, ny, nx]")
    filled = torch.zeros((S, ny, nx), dtype=torch.uint8, device=n.device)
    rounds = np.zeros((S, 2), dtype=np.int32)
    ep = eikonal_params(grid, ball, max_rounds, _global_path, scheme=scheme)
    st = _lib.EikonalStats()
    torch.cuda.synchronize(n.device)               # the library works on the null stream
    with torch.cuda.device(n.device):
        check(lib().rtmi_eikonal_fill_dev(C.byref(ep), n.data_ptr(), S, sources.data_ptr(), n_src.data_ptr(), T.data_ptr(),
                                          rounds.ctypes.data_as(_lib._ip), filled.data_ptr(), C.byref(st)))
    res = {"T": T, "rounds": rounds[:, 0].copy(), "converged": rounds[:, 1].copy(), "filled": filled}
    if stats:
        res["stats"] = eikonal_stats(st)
    return res


def _eikonal_lin_host(who, field_or_n, sources, grid, fill_result, n_src):
    """(n, src, n_src, T, filled, shape) of a host call of the linearised fill, contiguous and checked"""
    src = np.ascontiguousarray(np.asarray(sources, dtype=np.float64).reshape(-1, 2))
    S, nx, ny = len(src), int(grid[2]), int(grid[5])
    n, n_src = _eikonal_medium(who, field_or_n, src, grid, n_src)
    n = np.ascontiguousarray(n, dtype=np.float64)
    ns = np.ascontiguousarray(n_src, dtype=np.float64).reshape(-1)
    shape = (S, max(ny, 0), max(nx, 0))
    if nx >= 1 and ny >= 1 and n.shape != (ny, nx):
        raise ValueError(f"{who}: n must be [ny, nx] of the grid")
    if len(ns) != S:
        raise ValueError(f"{who}: n_src must be [S]")
    T = np.ascontiguousarray(fill_result["T"], dtype=np.float64)
    filled = np.ascontiguousarray(fill_result["filled"], dtype=np.uint8)
    if T.shape != shape or filled.shape != shape:
        raise ValueError(f"{who}: fill_result's T and filled must be [S, ny, nx]")
    return n, src, ns, T, filled, shape


def _eikonal_lin_array(who, name, a, shape):
    """a as a contiguous fp64 array of `shape`, or None"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"{who}: {name} must be {list(shape)}")
    return a


def eikonal_tangent(field_or_n, sources, grid, fill_result, dn, *, n_src=None, dn_src=None, dT_seed=None, ball=2.0, max_rounds=0,
                    stats=False, linearise="plain", _global_path=False):
    """The tangent of the eikonal fill, dT = J dn, on the device (rtmi_eikonal_tangent, include/rtmi.h): what a
    perturbation dn [ny, nx] of the slowness at the nodes, dn_src [S] of the slowness at the sources (None: 0) and dT_seed
    [S, ny, nx] of the seeds (None: 0) does to the table that eikonal_fill returned.  field_or_n, sources, grid, n_src, ball as in
    the eikonal_fill call that gave fill_result (its dict: T and filled are read).  Returns a dict: dT [S, ny, nx] (0 at
    obstacles and unreached nodes, dT_seed at seeds), rounds and converged [S], and with stats=True 'stats'.  Where converged
    is 0 the values are not final: raise max_rounds.  linearise="factored"  linearises the factored update, for a
    fill_result of eikonal_fill(scheme="factored"): the plain linearisation of such a table is off by 1 to 10 % of the largest
    |dT|, and by its own size in dn_src; some ten rounds in place of two or three.  The default "plain" keeps every bit.  The
    same argument on eikonal_adjoint, the _multi and _device forms and eikonal_operator."""
    who = "eikonal_tangent"
    n, src, ns, T, filled, shape = _eikonal_lin_host(who, field_or_n, sources, grid, fill_result, n_src)
    S = shape[0]
    dn = _eikonal_lin_array(who, "dn", dn, shape[1:])
    dn_src = _eikonal_lin_array(who, "dn_src", dn_src, (S,))
    dT_seed = _eikonal_lin_array(who, "dT_seed", dT_seed, shape)
    dT = np.zeros(shape)
    rounds = np.zeros((S, 2), dtype=np.int32)
    ep = eikonal_params(grid, ball, max_rounds, _global_path, linearise=linearise)
    st = _lib.EikonalStats()
    check(lib().rtmi_eikonal_tangent(C.byref(ep), dptr(n), S, dptr(src), dptr(ns), dptr(T), filled.ctypes.data_as(C.POINTER(C.c_uint8)),
                                     dptr(dn), dptr(dn_src), dptr(dT_seed), dptr(dT), rounds.ctypes.data_as(_lib._ip), C.byref(st)))
    res = {"dT": dT, "rounds": rounds[:, 0].copy(), "converged": rounds[:, 1].copy()}
    if stats:
        res["stats"] = eikonal_stats(st)
    return res


def eikonal_adjoint(field_or_n, sources, grid, fill_result, r, *, n_src=None, ball=2.0, max_rounds=0, stats=False,
                    linearise="plain", _global_path=False):
    """The adjoint of the eikonal fill, g = J^T r, on the device (rtmi_eikonal_adjoint): the gradient with respect to
    the medium of any misfit of the table whose derivative with respect to T is r [S, ny, nx] (ignored at obstacles and
    unreached nodes), by the adjoint-state method, with no rays.  Arguments as in eikonal_tangent.  Returns a dict:
      g [S, ny, nx]      the gradient with respect to n at the nodes, per source (sum over the sources for the whole misfit)
      g_src [S]          the gradient with respect to n_src
      lam [S, ny, nx]    the adjoint state; at a seed it is the gradient with respect to the seed's T
      rounds, converged  [S], as in eikonal_tangent
    and with stats=True 'stats'."""
    who = "eikonal_adjoint"
    n, src, ns, T, filled, shape = _eikonal_lin_host(who, field_or_n, sources, grid, fill_result, n_src)
    S = shape[0]
    r = _eikonal_lin_array(who, "r", r, shape)
    lam, g, g_src = np.zeros(shape), np.zeros(shape), np.zeros(S)
    rounds = np.zeros((S, 2), dtype=np.int32)
    ep = eikonal_params(grid, ball, max_rounds, _global_path, linearise=linearise)
    st = _lib.EikonalStats()
    check(lib().rtmi_eikonal_adjoint(C.byref(ep), dptr(n), S, dptr(src), dptr(ns), dptr(T), filled.ctypes.data_as(C.POINTER(C.c_uint8)),
                                     dptr(r), dptr(lam), dptr(g), dptr(g_src), rounds.ctypes.data_as(_lib._ip), C.byref(st)))
    res = {"lam": lam, "g": g, "g_src": g_src, "rounds": rounds[:, 0].copy(), "converged": rounds[:, 1].copy()}
    if stats:
        res["stats"] = eikonal_stats(st)
    return res


def _eikonal_lin_tensors(who, tensors):
    """Check the torch tensors of a device call of the linearised fill: (name, tensor or None, dtype, shape) each"""
    import torch
    device = None
    for name, a, dtype, shape in tensors:
        if a is None:
            continue
        if not isinstance(a, torch.Tensor):
            raise TypeError(f"{who}: {name} must be a torch tensor")
        if a.dtype != dtype:
            raise TypeError(f"{who}: {name} must be {dtype}")
        if not a.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous")
        if not a.is_cuda:
            raise ValueError(f"{who}: {name} must be a tensor on a GPU, not on the host")
        if device is not None and a.device != device:
            raise ValueError(f"{who}: {name} is on another device than n")
        device = a.device
        if tuple(a.shape) != shape:
            raise ValueError(f"{who}: {name} must be {list(shape)}")


def eikonal_tangent_device(n, sources, grid, fill_result, dn, *, n_src, dn_src=None, dT_seed=None, ball=2.0, max_rounds=0,
                           stats=False, linearise="plain", _global_path=False):
    """eikonal_tangent on torch tensors of one GPU, with no host copy (rtmi_eikonal_tangent_dev): n and dn [ny, nx], sources
    [S, 2], n_src and dn_src [S], dT_seed [S, ny, nx] in fp64, contiguous; fill_result is eikonal_fill_device's dict (T fp64,
    filled uint8, on the device).  dT is a new tensor on the device; rounds and converged are numpy arrays.  The same bits."""
    import torch
    who = "eikonal_tangent_device"
    if not isinstance(sources, torch.Tensor) or sources.dim() != 2:
        raise ValueError(f"{who}: sources must be a torch tensor [S, 2]")
    S, nx, ny = sources.shape[0], int(grid[2]), int(grid[5])
    f64 = torch.float64
    _eikonal_lin_tensors(who, [("n", n, f64, (ny, nx)), ("sources", sources, f64, (S, 2)), ("n_src", n_src, f64, (S,)),
                               ("T", fill_result["T"], f64, (S, ny, nx)), ("filled", fill_result["filled"], torch.uint8, (S, ny, nx)),
                               ("dn", dn, f64, (ny, nx)), ("dn_src", dn_src, f64, (S,)), ("dT_seed", dT_seed, f64, (S, ny, nx))])
    dT = torch.zeros((S, ny, nx), dtype=f64, device=n.device)
    rounds = np.zeros((S, 2), dtype=np.int32)
    ep = eikonal_params(grid, ball, max_rounds, _global_path, linearise=linearise)
    st = _lib.EikonalStats()
    opt = lambda a: None if a is None else a.data_ptr()      # noqa: E731
    torch.cuda.synchronize(n.device)               # the library works on the null stream
    with torch.cuda.device(n.device):
        check(lib().rtmi_eikonal_tangent_dev(C.byref(ep), n.data_ptr(), S, sources.data_ptr(), n_src.data_ptr(),
                                             fill_result["T"].data_ptr(), fill_result["filled"].data_ptr(), dn.data_ptr(), opt(dn_src),
                                             opt(dT_seed), dT.data_ptr(), rounds.ctypes.data_as(_lib._ip), C.byref(st)))
    res = {"dT": dT, "rounds": rounds[:, 0].copy(), "converged": rounds[:, 1].copy()}
    if stats:
        res["stats"] = eikonal_stats(st)
    return res


def eikonal_adjoint_device(n, sources, grid, fill_result, r, *, n_src, ball=2.0, max_rounds=0, stats=False,
                           linearise="plain", _global_path=False):
    """eikonal_adjoint on torch tensors of one GPU (rtmi_eikonal_adjoint_dev): arguments as in eikonal_tangent_device, r
    [S, ny, nx].  lam, g and g_src are new tensors on the device; rounds and converged are numpy arrays.  The same bits."""
    import torch
    who = "eikonal_adjoint_device"
    if not isinstance(sources, torch.Tensor) or sources.dim() != 2:
        raise ValueError(f"{who}: sources must be a torch tensor [S, 2]")
    S, nx, ny = sources.shape[0], int(grid[2]), int(grid[5])
    f64 = torch.float64
    _eikonal_lin_tensors(who, [("n", n, f64, (ny, nx)), ("sources", sources, f64, (S, 2)), ("n_src", n_src, f64, (S,)),
                               ("T", fill_result["T"], f64, (S, ny, nx)), ("filled", fill_result["filled"], torch.uint8, (S, ny, nx)),
                               ("r", r, f64, (S, ny, nx))])
    lam = torch.zeros((S, ny, nx), dtype=f64, device=n.device)
    g = torch.zeros((S, ny, nx), dtype=f64, device=n.device)
    g_src = torch.zeros((S,), dtype=f64, device=n.device)
    rounds = np.zeros((S, 2), dtype=np.int32)
    ep = eikonal_params(grid, ball, max_rounds, _global_path, linearise=linearise)
    st = _lib.EikonalStats()
    torch.cuda.synchronize(n.device)               # the library works on the null stream
    with torch.cuda.device(n.device):
        check(lib().rtmi_eikonal_adjoint_dev(C.byref(ep), n.data_ptr(), S, sources.data_ptr(), n_src.data_ptr(),
                                             fill_result["T"].data_ptr(), fill_result["filled"].data_ptr(), r.data_ptr(), lam.data_ptr(),
                                             g.data_ptr(), g_src.data_ptr(), rounds.ctypes.data_as(_lib._ip), C.byref(st)))
    res = {"lam": lam, "g": g, "g_src": g_src, "rounds": rounds[:, 0].copy(), "converged": rounds[:, 1].copy()}
    if stats:
        res["stats"] = eikonal_stats(st)
    return res


def eikonal_attributes(field_or_n, sources, grid, T, filled, theta0=None, theta=None, J=None, G=None, *, n_src=None, ball=2.0,
                       max_rounds=0, stats=False, _global_path=False):
    """Launch angle, arrival direction, spreading and amplitude factor at the nodes eikonal_fill gave a value, on the device
    (rtmi_eikonal_attributes, include/rtmi.h): what the rays know at the covered nodes -- theta0, theta, J, G
    [S, ny, nx] of the ray-cell table, NaN where no ray reaches; None: all NaN -- carried through the fill's causal network to the
    nodes `filled` marks, with no rays.  field_or_n, sources, grid, n_src, ball as in the eikonal_fill call that returned T and
    filled.  The inputs are not modified.  Returns a dict of [S, ny, nx] arrays: theta0, theta (arctan2(py, px) at the written
    nodes), px, py (the unit arrival direction, NaN at the nodes that were not written), J, G, and rounds, converged [S]; with
    stats=True also 'stats'.  Covered nodes keep their bits.  First order, like T: see DESIGN.md 38 for the figures, and shoot the
    full fan, since from the ball alone the launch angle is poor.  G spikes on the lines where two branches of the first arrival
    meet."""
    who = "eikonal_attributes"
    n, src, ns, T, filled, shape = _eikonal_lin_host(who, field_or_n, sources, grid, {"T": T, "filled": filled}, n_src)
    S = shape[0]
    cols = {}
    for name, a in (("theta0", theta0), ("theta", theta), ("J", J), ("G", G)):
        a = _eikonal_lin_array(who, name, a, shape)
        cols[name] = np.full(shape, np.nan) if a is None else a.copy()
    d = np.full((S, 2) + shape[1:], np.nan)
    rounds = np.zeros((S, 2), dtype=np.int32)
    ep = eikonal_params(grid, ball, max_rounds, _global_path)
    st = _lib.EikonalStats()
    check(lib().rtmi_eikonal_attributes(C.byref(ep), dptr(n), S, dptr(src), dptr(ns), dptr(T), filled.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        dptr(cols["theta0"]), dptr(d), dptr(cols["J"]), dptr(cols["G"]),
                                        rounds.ctypes.data_as(_lib._ip), C.byref(st)))
    px, py = d[:, 0].copy(), d[:, 1].copy()
    written = (filled != 0) & np.isfinite(T) & (np.isfinite(n) & (n > 0))[None]
    cols["theta"][written] = np.arctan2(py[written], px[written])
    res = {"theta0": cols["theta0"], "theta": cols["theta"], "px": px, "py": py, "J": cols["J"], "G": cols["G"],
           "rounds": rounds[:, 0].copy(), "converged": rounds[:, 1].copy()}
    if stats:
        res["stats"] = eikonal_stats(st)
    return res


def eikonal_attributes_device(n, sources, grid, T, filled, theta0=None, theta=None, J=None, G=None, *, n_src, ball=2.0, max_rounds=0,
                              stats=False, _global_path=False):
    """eikonal_attributes on torch tensors of one GPU, with no host copy of the tables (rtmi_eikonal_attributes_dev): n [ny, nx],
    sources [S, 2], n_src [S], T, theta0, theta, J, G [S, ny, nx] in fp64 and filled in uint8, contiguous.  theta0, theta, J and G
    are completed IN PLACE and returned; None: a new tensor from an all-NaN input.  px and py are new tensors; rounds and
    converged are numpy arrays.  The same bits."""
    import torch
    who = "eikonal_attributes_device"
    if not isinstance(sources, torch.Tensor) or sources.dim() != 2:
        raise ValueError(f"{who}: sources must be a torch tensor [S, 2]")
    S, nx, ny = sources.shape[0], int(grid[2]), int(grid[5])
    f64 = torch.float64
    tab = (S, ny, nx)
    _eikonal_lin_tensors(who, [("n", n, f64, (ny, nx)), ("sources", sources, f64, (S, 2)), ("n_src", n_src, f64, (S,)),
                               ("T", T, f64, tab), ("filled", filled, torch.uint8, tab), ("theta0", theta0, f64, tab),
                               ("theta", theta, f64, tab), ("J", J, f64, tab), ("G", G, f64, tab)])
    new = lambda a, shape=tab: torch.full(shape, float("nan"), dtype=f64, device=n.device) if a is None else a     # noqa: E731
    theta0, theta, J, G = new(theta0), new(theta), new(J), new(G)
    d = new(None, (S, 2, ny, nx))
    rounds = np.zeros((S, 2), dtype=np.int32)
    ep = eikonal_params(grid, ball, max_rounds, _global_path)
    st = _lib.EikonalStats()
    torch.cuda.synchronize(n.device)               # the library works on the null stream
    with torch.cuda.device(n.device):
        check(lib().rtmi_eikonal_attributes_dev(C.byref(ep), n.data_ptr(), S, sources.data_ptr(), n_src.data_ptr(), T.data_ptr(),
                                                filled.data_ptr(), theta0.data_ptr(), d.data_ptr(), J.data_ptr(), G.data_ptr(),
                                                rounds.ctypes.data_as(_lib._ip), C.byref(st)))
    px, py = d[:, 0].contiguous(), d[:, 1].contiguous()
    written = (filled != 0) & torch.isfinite(T) & (torch.isfinite(n) & (n > 0))[None]
    theta[written] = torch.atan2(py[written], px[written])
    res = {"theta0": theta0, "theta": theta, "px": px, "py": py, "J": J, "G": G, "rounds": rounds[:, 0].copy(),
           "converged": rounds[:, 1].copy()}
    if stats:
        res["stats"] = eikonal_stats(st)
    return res


def _eikonal_multi_result(out, rounds, st, stats):
    out["rounds"], out["converged"] = rounds[:, :, 0].copy(), rounds[:, :, 1].copy()
    if stats:
        out["stats"] = eikonal_stats(st)
    return out


def eikonal_tangent_multi(field_or_n, sources, grid, fill_result, dn, *, n_src=None, dn_src=None, dT_seed=None, ball=2.0,
                          max_rounds=0, stats=False, linearise="plain", _global_path=False, _width=0):
    """eikonal_tangent on K columns in one call (rtmi_eikonal_tangent_multi): dn [K, ny, nx], dn_src [K, S] or None,
    dT_seed [K, S, ny, nx] or None, 1 <= K <= 64.  Returns a dict: dT [K, S, ny, nx], rounds and converged [K, S], and with
    stats=True 'stats' (sums over the columns).  Column c has the bits of eikonal_tangent on column c alone."""
    who = "eikonal_tangent_multi"
    n, src, ns, T, filled, shape = _eikonal_lin_host(who, field_or_n, sources, grid, fill_result, n_src)
    S = shape[0]
    dn = np.ascontiguousarray(dn, dtype=np.float64)
    if dn.ndim != 3 or dn.shape[1:] != shape[1:]:
        raise ValueError(f"{who}: dn must be [K, ny, nx]")
    K = dn.shape[0]
    dn_src = _eikonal_lin_array(who, "dn_src", dn_src, (K, S))
    dT_seed = _eikonal_lin_array(who, "dT_seed", dT_seed, (K,) + shape)
    dT = np.zeros((K,) + shape)
    rounds = np.zeros((K, S, 2), dtype=np.int32)
    ep = eikonal_params(grid, ball, max_rounds, _global_path, _width, linearise=linearise)
    st = _lib.EikonalStats()
    check(lib().rtmi_eikonal_tangent_multi(C.byref(ep), dptr(n), S, dptr(src), dptr(ns), dptr(T),
                                           filled.ctypes.data_as(C.POINTER(C.c_uint8)), K, dptr(dn), dptr(dn_src), dptr(dT_seed),
                                           dptr(dT), rounds.ctypes.data_as(_lib._ip), C.byref(st)))
    return _eikonal_multi_result({"dT": dT}, rounds, st, stats)


def eikonal_adjoint_multi(field_or_n, sources, grid, fill_result, r, *, n_src=None, ball=2.0, max_rounds=0, stats=False,
                          linearise="plain", _global_path=False, _width=0):
    """eikonal_adjoint on K columns in one call (rtmi_eikonal_adjoint_multi): r [K, S, ny, nx], 1 <= K <= 64.
    Returns a dict: lam and g [K, S, ny, nx], g_src, rounds and converged [K, S], and with stats=True 'stats'.  Column c has the
    bits of eikonal_adjoint on column c alone."""
    who = "eikonal_adjoint_multi"
    n, src, ns, T, filled, shape = _eikonal_lin_host(who, field_or_n, sources, grid, fill_result, n_src)
    S = shape[0]
    r = np.ascontiguousarray(r, dtype=np.float64)
    if r.ndim != 4 or r.shape[1:] != shape:
        raise ValueError(f"{who}: r must be [K, S, ny, nx]")
    K = r.shape[0]
    lam, g, g_src = np.zeros((K,) + shape), np.zeros((K,) + shape), np.zeros((K, S))
    rounds = np.zeros((K, S, 2), dtype=np.int32)
    ep = eikonal_params(grid, ball, max_rounds, _global_path, _width, linearise=linearise)
    st = _lib.EikonalStats()
    check(lib().rtmi_eikonal_adjoint_multi(C.byref(ep), dptr(n), S, dptr(src), dptr(ns), dptr(T),
                                           filled.ctypes.data_as(C.POINTER(C.c_uint8)), K, dptr(r), dptr(lam), dptr(g), dptr(g_src),
                                           rounds.ctypes.data_as(_lib._ip), C.byref(st)))
    return _eikonal_multi_result({"lam": lam, "g": g, "g_src": g_src}, rounds, st, stats)


def eikonal_tangent_multi_device(n, sources, grid, fill_result, dn, *, n_src, dn_src=None, dT_seed=None, ball=2.0, max_rounds=0,
                                 stats=False, linearise="plain", _global_path=False, _width=0):
    """eikonal_tangent_multi on torch tensors of one GPU, with no host copy (rtmi_eikonal_tangent_multi_dev): as
    eikonal_tangent_device with dn [K, ny, nx], dn_src [K, S], dT_seed [K, S, ny, nx].  dT [K, S, ny, nx] is a new tensor on the
    device; rounds and converged [K, S] are numpy arrays.  The same bits."""
    import torch
    who = "eikonal_tangent_multi_device"
    if not isinstance(sources, torch.Tensor) or sources.dim() != 2:
        raise ValueError(f"{who}: sources must be a torch tensor [S, 2]")
    if not isinstance(dn, torch.Tensor) or dn.dim() != 3:
        raise ValueError(f"{who}: dn must be a torch tensor [K, ny, nx]")
    S, K, nx, ny = sources.shape[0], dn.shape[0], int(grid[2]), int(grid[5])
    f64 = torch.float64
    _eikonal_lin_tensors(who, [("n", n, f64, (ny, nx)), ("sources", sources, f64, (S, 2)), ("n_src", n_src, f64, (S,)),
                               ("T", fill_result["T"], f64, (S, ny, nx)), ("filled", fill_result["filled"], torch.uint8, (S, ny, nx)),
                               ("dn", dn, f64, (K, ny, nx)), ("dn_src", dn_src, f64, (K, S)),
                               ("dT_seed", dT_seed, f64, (K, S, ny, nx))])
    dT = torch.zeros((K, S, ny, nx), dtype=f64, device=n.device)
    rounds = np.zeros((K, S, 2), dtype=np.int32)
    ep = eikonal_params(grid, ball, max_rounds, _global_path, _width, linearise=linearise)
    st = _lib.EikonalStats()
    opt = lambda a: None if a is None else a.data_ptr()      # noqa: E731
    torch.cuda.synchronize(n.device)               # the library works on the null stream
    with torch.cuda.device(n.device):
        check(lib().rtmi_eikonal_tangent_multi_dev(C.byref(ep), n.data_ptr(), S, sources.data_ptr(), n_src.data_ptr(),
                                                   fill_result["T"].data_ptr(), fill_result["filled"].data_ptr(), K, dn.data_ptr(),
                                                   opt(dn_src), opt(dT_seed), dT.data_ptr(), rounds.ctypes.data_as(_lib._ip),
                                                   C.byref(st)))
    return _eikonal_multi_result({"dT": dT}, rounds, st, stats)


def eikonal_adjoint_multi_device(n, sources, grid, fill_result, r, *, n_src, ball=2.0, max_rounds=0, stats=False,
                                 linearise="plain", _global_path=False, _width=0):
    """eikonal_adjoint_multi on torch tensors of one GPU (rtmi_eikonal_adjoint_multi_dev): r [K, S, ny, nx].  lam, g
    [K, S, ny, nx] and g_src [K, S] are new tensors on the device; rounds and converged [K, S] are numpy arrays.  The same bits."""
    import torch
    who = "eikonal_adjoint_multi_device"
    if not isinstance(sources, torch.Tensor) or sources.dim() != 2:
        raise ValueError(f"{who}: sources must be a torch tensor [S, 2]")
    if not isinstance(r, torch.Tensor) or r.dim() != 4:
        raise ValueError(f"{who}: r must be a torch tensor [K, S, ny, nx]")
    S, K, nx, ny = sources.shape[0], r.shape[0], int(grid[2]), int(grid[5])
    f64 = torch.float64
    _eikonal_lin_tensors(who, [("n", n, f64, (ny, nx)), ("sources", sources, f64, (S, 2)), ("n_src", n_src, f64, (S,)),
                               ("T", fill_result["T"], f64, (S, ny, nx)), ("filled", fill_result["filled"], torch.uint8, (S, ny, nx)),
                               ("r", r, f64, (K, S, ny, nx))])
    lam = torch.zeros((K, S, ny, nx), dtype=f64, device=n.device)
    g = torch.zeros((K, S, ny, nx), dtype=f64, device=n.device)
    g_src = torch.zeros((K, S), dtype=f64, device=n.device)
    rounds = np.zeros((K, S, 2), dtype=np.int32)
    ep = eikonal_params(grid, ball, max_rounds, _global_path, _width, linearise=linearise)
    st = _lib.EikonalStats()
    torch.cuda.synchronize(n.device)               # the library works on the null stream
    with torch.cuda.device(n.device):
        check(lib().rtmi_eikonal_adjoint_multi_dev(C.byref(ep), n.data_ptr(), S, sources.data_ptr(), n_src.data_ptr(),
                                                   fill_result["T"].data_ptr(), fill_result["filled"].data_ptr(), K, r.data_ptr(),
                                                   lam.data_ptr(), g.data_ptr(), g_src.data_ptr(), rounds.ctypes.data_as(_lib._ip),
                                                   C.byref(st)))
    return _eikonal_multi_result({"lam": lam, "g": g, "g_src": g_src}, rounds, st, stats)


def eikonal_source_weights(sources, grid):
    """The bilinear weights of each source's cell: (idx [S, 4] node indices, w [S, 4]); w is all 0 for a source outside the grid"""
    gx0, gdx, nx, gy0, gdy, ny = grid
    nx, ny = int(nx), int(ny)
    src = np.asarray(sources, dtype=np.float64).reshape(-1, 2)
    u, v = (src[:, 0] - float(gx0)) / float(gdx), (src[:, 1] - float(gy0)) / float(gdy)
    inside = (u >= 0) & (u <= nx - 1) & (v >= 0) & (v <= ny - 1)
    i0 = np.clip(np.floor(np.where(inside, u, 0.0)).astype(np.int64), 0, max(nx - 2, 0))
    j0 = np.clip(np.floor(np.where(inside, v, 0.0)).astype(np.int64), 0, max(ny - 2, 0))
    i1, j1 = np.minimum(i0 + 1, nx - 1), np.minimum(j0 + 1, ny - 1)
    fu, fv = np.where(i1 > i0, u - i0, 0.0), np.where(j1 > j0, v - j0, 0.0)
    idx = np.stack([j0 * nx + i0, j0 * nx + i1, j1 * nx + i0, j1 * nx + i1], axis=1)
    w = np.stack([(1 - fu) * (1 - fv), fu * (1 - fv), (1 - fu) * fv, fu * fv], axis=1) * inside[:, None]
    return idx, w


def eikonal_operator(field_or_n, sources, grid, fill_result, receivers, *, n_src=None, ball=2.0, max_rounds=0, linearise="plain"):
    """The Jacobian of the filled tables at receiver nodes as a scipy LinearOperator, matrix-free, for LSQR or Gauss-Newton
    (DESIGN.md 35): it maps dn [ny nx] to dT at `receivers` (node indices iy nx + ix, [R]) of every source; row s R + k is source
    s, receiver k.  matvec is eikonal_tangent_device and a gather; rmatvec a scatter, eikonal_adjoint_device and a sum over the
    sources.  n_src follows dn through the bilinear weights of the source's cell where the source lies inside the grid, else it
    is held fixed.  field_or_n, sources, grid, n_src, ball as in the eikonal_fill call that gave fill_result; everything is
    uploaded once.  A sweep that does not converge within max_rounds raises.  Receivers off the nodes: compose an interpolation.
    linearise as in eikonal_tangent."""
    import torch
    from scipy.sparse.linalg import LinearOperator
    who = "eikonal_operator"
    eikonal_params(grid, ball, max_rounds, linearise=linearise)        # refuses a bad linearise before anything is uploaded
    n, src, ns, T, filled, shape = _eikonal_lin_host(who, field_or_n, sources, grid, fill_result, n_src)
    S, ny, nx = shape
    rec = np.asarray(receivers, dtype=np.int64).reshape(-1)
    if len(rec) and (rec.min() < 0 or rec.max() >= ny * nx):
        raise ValueError(f"{who}: receivers must be node indices in [0, ny nx)")
    dev = torch.device("cuda")
    up = lambda a: torch.as_tensor(a, device=dev)      # noqa: E731
    d_n, d_src, d_ns, d_rec = up(n), up(src), up(ns), up(rec)
    d_fill = {"T": up(T), "filled": up(filled)}
    idx, w = eikonal_source_weights(src, grid)
    d_idx, d_w = up(idx), up(w)
    kw = dict(n_src=d_ns, ball=ball, max_rounds=max_rounds, linearise=linearise)

    def done(res, what):
        if not res["converged"].all():
            raise RuntimeError(f"{who}: the {what} sweeps did not converge within max_rounds")
        return res

    def matvec(x):
        d_dn = up(np.ascontiguousarray(x, dtype=np.float64).reshape(ny, nx))
        d_dns = (d_dn.reshape(-1)[d_idx] * d_w).sum(dim=1)
        res = done(eikonal_tangent_device(d_n, d_src, grid, d_fill, d_dn, dn_src=d_dns, **kw), "tangent")
        return res["dT"].reshape(S, -1)[:, d_rec].reshape(-1).cpu().numpy()

    def rmatvec(y):
        d_r = torch.zeros((S, ny * nx), dtype=torch.float64, device=dev)
        d_y = up(np.ascontiguousarray(y, dtype=np.float64).reshape(S, -1))
        d_r.index_put_((torch.arange(S, device=dev)[:, None].expand(S, len(rec)), d_rec[None, :].expand(S, len(rec))), d_y,
                       accumulate=True)
        res = done(eikonal_adjoint_device(d_n, d_src, grid, d_fill, d_r.reshape(S, ny, nx), **kw), "adjoint")
        g = res["g"].sum(dim=0).reshape(-1)
        g.index_put_((d_idx.reshape(-1),), (res["g_src"][:, None] * d_w).reshape(-1), accumulate=True)
        return g.cpu().numpy()

    return LinearOperator((S * len(rec), ny * nx), matvec=matvec, rmatvec=rmatvec, dtype=np.float64)


def eikonal_tomo_stats(st):
    return {"rows": int(st.rows), "live_rows": int(st.live_rows), "S": int(st.S), "R": int(st.R), "nx": int(st.nx), "ny": int(st.ny),
            "touched": int(st.touched), "bytes_device": int(st.bytes_device), "self_filled": bool(st.self_filled),
            "path": _lib.EIKONAL_PATHS.get(st.path, st.path), "rounds_max": int(st.rounds_max), "sweep_ms": st.sweep_ms,
            "kernel_ms": st.kernel_ms, "reduce_ms": st.reduce_ms}


class EikonalTomography:
    """First-arrival eikonal tomography that stays on the device (rtmi_eikonal_tomo_*, include/rtmi.h): the Jacobian
    of the filled tables at `receivers` [R, 2], coordinates anywhere on the grid, as a handle with two bit-defined products, the
    residual of picks, LSQR on the device and Gauss-Newton.  Row s R + k is source s, receiver k.  field_or_n, sources, grid,
    n_src, ball, max_rounds as in eikonal_fill.  fill_result: the dict of the eikonal_fill call that gave the tables (this is how
    a table seeded by rays enters); None: the handle fills its own from the ball, and only then can it be re-linearised.
    scheme "plain" or "factored"  is the scheme of that own fill and of every relinearise; it cannot be given
    together with fill_result, whose tables are already made.  linearise "plain" (the default, which keeps every bit) or
    "factored"  is the linearisation of apply, transpose, lsqr, their _multi forms and of every relinearise:
    "factored" is consistent with tables of the factored scheme, so it needs scheme="factored", or a fill_result that
    eikonal_fill(scheme="factored") made; "plain" linearises the plain update about the table, whatever filled it.
    n_src follows the model through the bilinear weights of the source's cell where the source lies inside the grid.  A row is
    live where none of the four nodes round its receiver is an obstacle or unreached; other rows read and give 0."""

    def __init__(self, field_or_n, sources, grid, receivers, *, fill_result=None, n_src=None, ball=2.0, max_rounds=0, scheme=None,
                 linearise="plain", _global_path=False, _width=0):
        who = "EikonalTomography"
        self._h = None
        if scheme is not None and fill_result is not None:
            raise ValueError(f"{who}: scheme is the scheme of the handle's own fill; it cannot be given together with fill_result")
        if linearise == "factored" and fill_result is None and scheme != "factored" and scheme in (None, "plain"):
            raise ValueError(f'{who}: linearise="factored" on a handle that fills its own tables needs scheme="factored"')
        src = np.ascontiguousarray(np.asarray(sources, dtype=np.float64).reshape(-1, 2))
        S, nx, ny = len(src), int(grid[2]), int(grid[5])
        n, ns = _eikonal_medium(who, field_or_n, src, grid, n_src)
        n = np.ascontiguousarray(n, dtype=np.float64)
        ns = np.ascontiguousarray(ns, dtype=np.float64).reshape(-1)
        if nx >= 1 and ny >= 1 and n.shape != (ny, nx):
            raise ValueError(f"{who}: n must be [ny, nx] of the grid")
        if len(ns) != S:
            raise ValueError(f"{who}: n_src must be [S]")
        rec = np.ascontiguousarray(np.asarray(receivers, dtype=np.float64).reshape(-1, 2))
        T = filled = None
        if fill_result is not None:
            T = np.ascontiguousarray(fill_result["T"], dtype=np.float64)
            filled = np.ascontiguousarray(fill_result["filled"], dtype=np.uint8)
            if T.shape != (S, ny, nx) or filled.shape != (S, ny, nx):
                raise ValueError(f"{who}: fill_result's T and filled must be [S, ny, nx]")
        self.grid, self.S, self.R, self.nx, self.ny = tuple(grid), S, len(rec), nx, ny
        self.n, self.sources, self.receivers = n.copy(), src, rec
        ep = eikonal_params(grid, ball, max_rounds, _global_path, _width, scheme="plain" if scheme is None else scheme,
                            linearise=linearise)
        h = C.c_void_p()
        check(lib().rtmi_eikonal_tomo_create(C.byref(ep), dptr(n), S, dptr(src), dptr(ns), dptr(T),
                                             None if filled is None else filled.ctypes.data_as(C.POINTER(C.c_uint8)), len(rec), dptr(rec),
                                             C.byref(h)))
        self._h = h

    def _open(self):
        if self._h is None:
            raise ValueError("EikonalTomography: the handle is closed")
        return self._h

    @property
    def shape(self):
        return (self.S * self.R, self.ny * self.nx)

    def info(self):
        """rows, live_rows, live_per_source [S], the shape, the nodes the receivers touch, the device bytes"""
        st = _lib.EikonalTomoStats()
        per = np.zeros(self.S, dtype=np.int64)
        check(lib().rtmi_eikonal_tomo_info(self._open(), C.byref(st), per.ctypes.data_as(C.POINTER(C.c_int64))))
        out = eikonal_tomo_stats(st)
        out["live_per_source"] = per
        return out

    def table(self):
        """The handle's tables: T [S, ny, nx], filled [S, ny, nx] uint8 and live [S, R] uint8"""
        T = np.empty((self.S, self.ny, self.nx))
        filled = np.empty((self.S, self.ny, self.nx), dtype=np.uint8)
        live = np.empty((self.S, self.R), dtype=np.uint8)
        u8 = C.POINTER(C.c_uint8)
        check(lib().rtmi_eikonal_tomo_table(self._open(), dptr(T), filled.ctypes.data_as(u8), live.ctypes.data_as(u8)))
        return {"T": T, "filled": filled, "live": live}

    def _host(self, who, a, size, name):
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        if a.size != size:
            raise ValueError(f"EikonalTomography.{who}: {name} must have {size} values")
        return a

    def _device(self, who, t, size, name):
        import torch
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.numel() != size:
            raise ValueError(f"EikonalTomography.{who}: {name} must be a contiguous fp64 torch tensor of {size} values on the GPU")
        torch.cuda.synchronize(t.device)               # the library works on the null stream
        return t

    def apply(self, dn, stats=False):
        """y [S R] = A dn for dn [ny, nx] (rtmi_eikonal_tomo_apply); a sweep that does not converge raises"""
        dn = self._host("apply", dn, self.ny * self.nx, "dn")
        y = np.empty(self.S * self.R)
        st = _lib.EikonalTomoStats()
        check(lib().rtmi_eikonal_tomo_apply(self._open(), dptr(dn), dptr(y), C.byref(st)))
        return (y, eikonal_tomo_stats(st)) if stats else y

    def transpose(self, y, stats=False):
        """G [ny, nx] = A^T y for y [S R] (rtmi_eikonal_tomo_transpose); a dead row's entry is not read"""
        y = self._host("transpose", y, self.S * self.R, "y")
        G = np.empty((self.ny, self.nx))
        st = _lib.EikonalTomoStats()
        check(lib().rtmi_eikonal_tomo_transpose(self._open(), dptr(y), dptr(G), C.byref(st)))
        return (G, eikonal_tomo_stats(st)) if stats else G

    def apply_device(self, dn, out=None, stats=False):
        """apply on torch tensors of the handle's device, with no host copy (rtmi_eikonal_tomo_apply_dev): the same bits"""
        import torch
        dn = self._device("apply_device", dn, self.ny * self.nx, "dn")
        y = torch.empty(self.S * self.R, dtype=torch.float64, device=dn.device) if out is None else self._device("apply_device", out, self.S * self.R, "out")
        st = _lib.EikonalTomoStats()
        with torch.cuda.device(dn.device):
            check(lib().rtmi_eikonal_tomo_apply_dev(self._open(), dn.data_ptr(), y.data_ptr(), C.byref(st)))
        return (y, eikonal_tomo_stats(st)) if stats else y

    def transpose_device(self, y, out=None, stats=False):
        """transpose on torch tensors of the handle's device (rtmi_eikonal_tomo_transpose_dev): the same bits"""
        import torch
        y = self._device("transpose_device", y, self.S * self.R, "y")
        G = (torch.empty((self.ny, self.nx), dtype=torch.float64, device=y.device) if out is None
             else self._device("transpose_device", out, self.ny * self.nx, "out"))
        st = _lib.EikonalTomoStats()
        with torch.cuda.device(y.device):
            check(lib().rtmi_eikonal_tomo_transpose_dev(self._open(), y.data_ptr(), G.data_ptr(), C.byref(st)))
        return (G, eikonal_tomo_stats(st)) if stats else G

    def residual(self, picks):
        """res [S R] = picks - the tables sampled at the receivers; +0.0 on a dead row and where the pick is NaN (absent)"""
        picks = self._host("residual", picks, self.S * self.R, "picks")
        res = np.empty(self.S * self.R)
        check(lib().rtmi_eikonal_tomo_residual(self._open(), dptr(picks), dptr(res)))
        return res

    def residual_device(self, picks):
        import torch
        picks = self._device("residual_device", picks, self.S * self.R, "picks")
        res = torch.empty(self.S * self.R, dtype=torch.float64, device=picks.device)
        with torch.cuda.device(picks.device):
            check(lib().rtmi_eikonal_tomo_residual_dev(self._open(), picks.data_ptr(), res.data_ptr()))
        return res

    def lsqr(self, rhs, iter_lim, damp=0.0, atol=0.0, btol=0.0, row_weight=None, col_scale=None, x0=None, smooth=None, smooth2=None,
             history=False, stats=False):
        """rtmi_eikonal_tomo_lsqr: min |W A D y - W (rhs - A x0)|^2 + damp^2 |y|^2 + the smoothing rows of D y on the node grid,
        x = x0 + D y, every vector on the device.  smooth = (lx, ly), smooth2 = (mx2, my2) as in Tomography.lsqr.  row_weight
        [S R] must be 0 on dead rows; col_scale and x0 [ny, nx].  -> the dict of Tomography.lsqr with x [ny, nx]."""
        who = "EikonalTomography.lsqr"
        rr = self._host("lsqr", rhs, self.S * self.R, "rhs")
        iter_lim = int(iter_lim)
        if iter_lim < 1:
            raise ValueError(f"{who}: iter_lim must be >= 1")
        lp = _lib.LsqrParams()
        lp.iter_lim, lp.damp, lp.atol, lp.btol = iter_lim, float(damp), float(atol), float(btol)
        reg = None
        if smooth is not None or smooth2 is not None:
            reg = _lib.TomoReg()
            for name, pair, dst in (("smooth", smooth, reg.d1), ("smooth2", smooth2, reg.d2)):
                if pair is not None:
                    pp = np.ascontiguousarray(pair, dtype=np.float64)
                    if pp.shape != (2,):
                        raise ValueError(f"{who}: {name} must be a pair")
                    dst[0], dst[1] = pp
        lo = keep = None
        if row_weight is not None or col_scale is not None or x0 is not None:
            lo, keep = _lsqr_options(who, rr.size, self.ny * self.nx, row_weight, col_scale, x0)
        x = np.empty((self.ny, self.nx))
        hist = np.zeros((iter_lim, 4)) if history else None
        st = _lib.LsqrStats()
        check(lib().rtmi_eikonal_tomo_lsqr(self._open(), C.byref(lp), None if lo is None else C.byref(lo),
                                           None if reg is None else C.byref(reg), dptr(rr), dptr(x), dptr(hist), C.byref(st)))
        out = {"x": x, "istop": int(st.istop), "itn": int(st.itn), "r1norm": st.r1norm, "r2norm": st.r2norm, "anorm": st.anorm,
               "arnorm": st.arnorm}
        if history:
            out["history"] = hist[:st.itn].copy()
        if stats:
            out["stats"] = {"total_ms": st.total_ms, "operator_ms": st.operator_ms, "vector_ms": st.vector_ms,
                            "bytes_device": int(st.bytes_device)}
        return out

    # ------------------------------------------------------------------------------------------ several columns
    def set_column_group(self, cg):
        """The columns the batched calls sweep together (rtmi_eikonal_tomo_set_column_group); 0: the default, as many as keep the
        work tables under 8 GiB.  For callers short of memory; no result depends on it."""
        check(lib().rtmi_eikonal_tomo_set_column_group(self._open(), int(cg)))

    def _columns(self, who, a, per, name, shape):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim < 2 or a.shape[1:] not in ((per,), shape):
            raise ValueError(f"EikonalTomography.{who}: {name} must be [K, {', '.join(str(v) for v in shape)}]")
        return a.reshape(a.shape[0], per)

    def _multi(self, fn, a, per_out, stats):
        """one C call per group of at most 64 columns"""
        K = a.shape[0]
        out = np.empty((K, per_out))
        sts = []
        for lo in range(0, K, _lib.LSQR_MULTI_MAX):
            hi = min(K, lo + _lib.LSQR_MULTI_MAX)
            part, res = np.ascontiguousarray(a[lo:hi]), np.empty((hi - lo, per_out))
            st = _lib.EikonalTomoStats()
            check(fn(self._open(), hi - lo, dptr(part), dptr(res), C.byref(st)))
            out[lo:hi] = res
            sts.append(eikonal_tomo_stats(st))
        return (out, sts) if stats else out

    def matmat(self, X, stats=False):
        """Y [K, S R] = A X for X [K, ny, nx] (rtmi_eikonal_tomo_apply_multi): column c has the bits of apply(X[c]).  Any K, in
        groups of at most 64.  With stats=True -> (Y, the groups' stats)."""
        X = self._columns("matmat", X, self.ny * self.nx, "X", (self.ny, self.nx))
        return self._multi(lib().rtmi_eikonal_tomo_apply_multi, X, self.S * self.R, stats)

    def rmatmat(self, Y, stats=False):
        """G [K, ny, nx] = A^T Y for Y [K, S R] (rtmi_eikonal_tomo_transpose_multi): column c has the bits of transpose(Y[c])"""
        Y = self._columns("rmatmat", Y, self.S * self.R, "Y", (self.S * self.R,))
        res = self._multi(lib().rtmi_eikonal_tomo_transpose_multi, Y, self.ny * self.nx, stats)
        G = (res[0] if stats else res).reshape(-1, self.ny, self.nx)
        return (G, res[1]) if stats else G

    def _multi_device(self, who, fn, t, per_in, per_out, out, stats):
        import torch
        if not isinstance(t, torch.Tensor) or t.dim() < 2:
            raise ValueError(f"EikonalTomography.{who}: the input must be a torch tensor [K, ...]")
        K = t.shape[0]
        if not 1 <= K <= _lib.LSQR_MULTI_MAX:
            raise ValueError(f"EikonalTomography.{who}: K must be in 1 .. {_lib.LSQR_MULTI_MAX}")
        t = self._device(who, t, K * per_in, "the input")
        res = torch.empty((K, per_out), dtype=torch.float64, device=t.device) if out is None else self._device(who, out, K * per_out, "out")
        st = _lib.EikonalTomoStats()
        with torch.cuda.device(t.device):
            check(fn(self._open(), K, t.data_ptr(), res.data_ptr(), C.byref(st)))
        return (res, eikonal_tomo_stats(st)) if stats else res

    def matmat_device(self, X, out=None, stats=False):
        """matmat on torch tensors of the handle's device, with no host copy (rtmi_eikonal_tomo_apply_multi_dev), K <= 64"""
        return self._multi_device("matmat_device", lib().rtmi_eikonal_tomo_apply_multi_dev, X, self.ny * self.nx, self.S * self.R, out, stats)

    def rmatmat_device(self, Y, out=None, stats=False):
        """rmatmat on torch tensors of the handle's device (rtmi_eikonal_tomo_transpose_multi_dev), K <= 64 -> [K, ny, nx]"""
        res = self._multi_device("rmatmat_device", lib().rtmi_eikonal_tomo_transpose_multi_dev, Y, self.S * self.R, self.ny * self.nx, out,
                                 stats)
        G = (res[0] if stats else res).reshape(-1, self.ny, self.nx)
        return (G, res[1]) if stats else G

    def lsqr_multi(self, rhs, iter_lim, damp=0.0, atol=0.0, btol=0.0, row_weight=None, col_scale=None, x0=None, smooth=None, smooth2=None,
                   history=False, stats=False, group=None):
        """rtmi_eikonal_tomo_lsqr_multi: lsqr for the K right-hand sides rhs [K, S R] in lock-step -> a list of K dicts of lsqr's
        shape, each with the bits of lsqr(rhs[c], ...).  The keywords are lsqr's; col_scale and x0 are shared, row_weight is
        [S R] for all or [K, S R], one weighting per column.  Any K: in groups of at most 64 columns, or of `group`."""
        who = "EikonalTomography.lsqr_multi"
        rows, nm = self.S * self.R, self.ny * self.nx
        rr = np.ascontiguousarray(rhs, dtype=np.float64)
        if rr.ndim != 2 or rr.shape[1] != rows:
            raise ValueError(f"{who}: rhs must be [K, {rows}]")
        K = rr.shape[0]
        iter_lim = int(iter_lim)
        if iter_lim < 1:
            raise ValueError(f"{who}: iter_lim must be >= 1")
        group = _lib.LSQR_MULTI_MAX if group is None else int(group)
        if not 1 <= group <= _lib.LSQR_MULTI_MAX:
            raise ValueError(f"{who}: group must be in 1 .. {_lib.LSQR_MULTI_MAX}")
        lp = _lib.LsqrParams()
        lp.iter_lim, lp.damp, lp.atol, lp.btol = iter_lim, float(damp), float(atol), float(btol)
        reg = None
        if smooth is not None or smooth2 is not None:
            reg = _lib.TomoReg()
            for name, pair, dst in (("smooth", smooth, reg.d1), ("smooth2", smooth2, reg.d2)):
                if pair is not None:
                    pp = np.ascontiguousarray(pair, dtype=np.float64)
                    if pp.shape != (2,):
                        raise ValueError(f"{who}: {name} must be a pair")
                    dst[0], dst[1] = pp
        wr, flags = None, 0
        if row_weight is not None:
            wr = np.ascontiguousarray(row_weight, dtype=np.float64)
            if wr.ndim == 2 and wr.shape == (K, rows) and K != 1:
                flags = _lib.LSQR_MULTI_ROW_WEIGHT
            elif wr.size == rows:
                wr = wr.reshape(rows)
            else:
                raise ValueError(f"{who}: row_weight must be [{rows}] or [K, {rows}]")
        lo = keep = None
        if wr is not None or col_scale is not None or x0 is not None:
            lo, keep = _lsqr_options(who, rows, nm, None, col_scale, x0)
        out = []
        for a in range(0, K, group):
            b = min(K, a + group)
            n = b - a
            x = np.empty((n, self.ny, self.nx))
            hist = np.zeros((n, iter_lim, 4)) if history else None
            st = (_lib.LsqrStats * n)()
            if wr is not None:
                wg = np.ascontiguousarray(wr[a:b]) if flags else wr
                lo.row_weight = dptr(wg)
            check(lib().rtmi_eikonal_tomo_lsqr_multi(self._open(), C.byref(lp), None if lo is None else C.byref(lo),
                                                     None if reg is None else C.byref(reg), n, flags, dptr(np.ascontiguousarray(rr[a:b])),
                                                     dptr(x), dptr(hist), st))
            for s in range(n):
                o = {"x": x[s], "istop": int(st[s].istop), "itn": int(st[s].itn), "r1norm": st[s].r1norm, "r2norm": st[s].r2norm,
                     "anorm": st[s].anorm, "arnorm": st[s].arnorm}
                if history:
                    o["history"] = hist[s, :st[s].itn].copy()
                if stats:
                    o["stats"] = {"total_ms": st[s].total_ms, "operator_ms": st[s].operator_ms, "vector_ms": st[s].vector_ms,
                                  "bytes_device": int(st[s].bytes_device)}
                out.append(o)
        return out

    def recover(self, models, **lsqr_kw):
        """The resolution test: d_c = A m_c (matmat), then lsqr_multi(d, **lsqr_kw) -> (the recovered models [K, ny, nx], the
        dicts).  models [K, ny, nx], e.g. checkerboard(...) or spikes(...) stacked."""
        mm = np.ascontiguousarray(models, dtype=np.float64)
        if mm.ndim != 3 or mm.shape[1:] != (self.ny, self.nx):
            raise ValueError(f"EikonalTomography.recover: models must be [K, {self.ny}, {self.nx}]")
        outs = self.lsqr_multi(self.matmat(mm), **lsqr_kw)
        return np.stack([o["x"] for o in outs]) if outs else np.empty((0, self.ny, self.nx)), outs

    def bootstrap(self, rhs, n, seed, results=False, **lsqr_kw):
        """n bootstrap replicates of lsqr(rhs, ...): replicate k weighs row r by the square root of its multiplicity in a draw of
        S R rows with replacement (bootstrap_weights(S R, n, seed)), zeroed on dead rows, times the caller's row_weight [S R], if
        given; one lsqr_multi over them.  -> (mean, standard deviation with ddof 1) of x over the replicates, [ny, nx] each, and
        with results=True the per-replicate dicts as well."""
        rows = self.S * self.R
        rr = np.ascontiguousarray(rhs, dtype=np.float64).reshape(-1)
        if rr.size != rows:
            raise ValueError(f"EikonalTomography.bootstrap: rhs must have {rows} values")
        w = bootstrap_weights(rows, n, seed) * (self.table()["live"].reshape(-1) != 0)[None, :]
        base = lsqr_kw.pop("row_weight", None)
        if base is not None:
            bb = np.ascontiguousarray(base, dtype=np.float64).reshape(-1)
            if bb.size != rows:
                raise ValueError(f"EikonalTomography.bootstrap: row_weight must have {rows} values")
            w = w * bb[None, :]
        outs = self.lsqr_multi(np.broadcast_to(rr, (len(w), rows)), row_weight=w, **lsqr_kw)
        xs = np.stack([o["x"] for o in outs])
        mean, std = xs.mean(axis=0), xs.std(axis=0, ddof=1)
        return (mean, std, outs) if results else (mean, std)

    def as_linear_operator(self):
        """A scipy LinearOperator [S R, ny nx] over apply and transpose (host vectors: two PCIe crossings per product)"""
        from scipy.sparse.linalg import LinearOperator
        return LinearOperator(self.shape, matvec=self.apply, rmatvec=lambda y: self.transpose(y).reshape(-1), dtype=np.float64)

    def relinearise(self, n, n_src=None):
        """A new medium n [ny, nx] for a handle that filled its own tables: they are filled again on the device and the live rows
        found again (rtmi_eikonal_tomo_relinearise).  n_src [S] or None: a source inside the grid gets n sampled at it."""
        n = self._host("relinearise", n, self.ny * self.nx, "n")
        ns = None if n_src is None else self._host("relinearise", n_src, self.S, "n_src")
        check(lib().rtmi_eikonal_tomo_relinearise(self._open(), dptr(n), dptr(ns)))
        self.n = n.reshape(self.ny, self.nx).copy()

    def relinearise_device(self, n, n_src=None):
        """relinearise on torch tensors of the handle's device (rtmi_eikonal_tomo_relinearise_dev): the same bits"""
        import torch
        n = self._device("relinearise_device", n, self.ny * self.nx, "n")
        if n_src is not None:
            n_src = self._device("relinearise_device", n_src, self.S, "n_src")
        with torch.cuda.device(n.device):
            check(lib().rtmi_eikonal_tomo_relinearise_dev(self._open(), n.data_ptr(), None if n_src is None else n_src.data_ptr()))
        self.n = n.detach().cpu().numpy().reshape(self.ny, self.nx).copy()

    def gauss_newton(self, picks, iters, **lsqr_kw):
        """iters times: residual, lsqr, n += x, relinearise.  picks [S R], NaN where absent.  lsqr_kw: the keywords of lsqr
        (iter_lim too; 30 if absent).  On each step col_scale defaults to 0 at obstacle nodes and 1 elsewhere, and row_weight is
        0 on dead rows and absent picks (a given row_weight is multiplied by that mask).  Raises if a step would make n <= 0 at
        a node that is no obstacle.  -> {"n": the last model, "rms": [iters + 1] the rms residual of every model over the rows in
        use, "steps": the lsqr dicts}"""
        who = "EikonalTomography.gauss_newton"
        picks = self._host("gauss_newton", picks, self.S * self.R, "picks")
        kw = dict(lsqr_kw)
        iter_lim = kw.pop("iter_lim", 30)
        given_w = kw.pop("row_weight", None)
        given_c = kw.pop("col_scale", None)
        present = ~np.isnan(picks)
        rms, steps = [], []

        def measure():
            res = self.residual(picks)
            used = present & (self.table()["live"].reshape(-1) != 0)
            rms.append(float(np.sqrt((res * res).sum() / max(int(used.sum()), 1))))
            return res, used

        for _ in range(int(iters)):
            res, used = measure()
            open_ = np.isfinite(self.n) & (self.n > 0)
            w = used.astype(np.float64) if given_w is None else np.asarray(given_w, dtype=np.float64).reshape(-1) * used
            c = open_.astype(np.float64) if given_c is None else given_c
            out = self.lsqr(res, iter_lim, row_weight=w, col_scale=c, **kw)
            n1 = self.n + out["x"]
            if (n1[open_] <= 0).any():
                raise ValueError(f"{who}: the step would make n <= 0 at a node that is no obstacle (more damping or smoothing)")
            self.relinearise(n1)
            steps.append(out)
        measure()
        return {"n": self.n.copy(), "rms": np.array(rms), "steps": steps}

    def close(self):
        if self._h is not None:
            lib().rtmi_eikonal_tomo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def beam_params(grid, eps, cutoff=None, max_width=None, edge_taper=0):
    """rtmi_beam_params of grid = (gx0, gdx, nx, gy0, gdy, ny) and the beam parameter eps; None / 0 take the library's defaults"""
    gx0, gdx, nx, gy0, gdy, ny = grid
    bp = _lib.BeamParams()
    bp.gx0 = float(gx0); bp.gdx = float(gdx); bp.nx = int(nx)
    bp.gy0 = float(gy0); bp.gdy = float(gdy); bp.ny = int(ny)
    bp.eps = float(eps); bp.cutoff = float(cutoff or 0.0); bp.max_width = float(max_width or 0.0)
    bp.edge_taper = float(edge_taper or 0.0)
    return bp


def beam_stats(st):
    return {"segments": st.segments, "tile_entries": st.tile_entries, "pairs_tested": st.pairs_tested,
            "pairs_inside": st.pairs_inside, "capped": st.capped, "prep_ms": st.prep_ms, "bin_ms": st.bin_ms,
            "gather_ms": st.gather_ms, "cutoff": st.cutoff, "max_width": st.max_width}


def _beam_call(call, S, grid, omegas, eps, cutoff, max_width, edge_taper, stats):
    bp = beam_params(grid, eps, cutoff, max_width, edge_taper)
    om = np.ascontiguousarray(np.atleast_1d(omegas), dtype=np.float64)
    nx, ny = max(int(bp.nx), 0), max(int(bp.ny), 0)
    u = np.zeros((max(S, 0), len(om), ny, nx, 2))
    st = _lib.BeamStats()
    check(call(C.byref(bp), len(om), dptr(om), dptr(u), C.byref(st)))
    u = u[..., 0] + 1j * u[..., 1]
    return (u, beam_stats(st)) if stats else u


def beam_table(selected_func, field, sources, grid, omegas, *, thetas, eps, step, max_size, box, gamma=1, mem_budget=0,
               cutoff=None, max_width=None, edge_taper=0, stats=False, **batch_kw):
    """Gaussian-beam wavefields from many sources onto one grid, by public calls only: traveltime_table's count
    pass and memory-bounded source groups, then Batch.gaussian_beams per group.  Per row and ray a group holds the record (48
    bytes in fp64, 24 in fp32) and the beam pass's own 144 (Q1 P1 Q2 P2 n and eleven per-row values), under mem_budget (default
    8 GiB).  Each source's field depends on its own rays only, so the grouping changes no bit.  Returns complex128
    [S, nw, ny, nx]; with stats=True (u, stats): rec_rows, groups, count_ms, trace_ms, beam_ms (host wall times) and the beam
    calls' summed counters."""
    src = np.asarray(sources, dtype=np.float64).reshape(-1, 2)
    th = np.ascontiguousarray(thetas, dtype=np.float64)
    S, M = len(src), len(th)
    batch_kw = dict(batch_kw)
    batch_kw.pop("keep_n_ray", None)
    t0 = time.perf_counter()
    c = Batch(field, selected_func, step, max_size, box, gamma, np.tile(th, S), np.repeat(src[:, 0], M), np.repeat(src[:, 1], M),
              record_stride=0, keep_n_ray=False, **batch_kw)
    try:
        c.run()
        rows = int(c.d_ray()[2].max()) + 1
    finally:
        c.close()
    t1 = time.perf_counter()
    per_ray = rows * ((48 if field.dtype == F64 else 24) + 144)
    budget = int(mem_budget) if mem_budget else 8 << 30
    G = max(1, min(S, budget // max(per_ray * M, 1)))
    res, tot = None, {"rec_rows": rows, "groups": 0, "count_ms": (t1 - t0) * 1e3, "trace_ms": 0.0, "beam_ms": 0.0}
    for g0 in range(0, S, G):
        sg = src[g0:g0 + G]
        ta = time.perf_counter()
        b = Batch(field, selected_func, step, max_size, box, gamma, np.tile(th, len(sg)), np.repeat(sg[:, 0], M),
                  np.repeat(sg[:, 1], M), record_stride=1, rec_rows=rows, keep_n_ray=False, **batch_kw)
        try:
            b.run()
            b.sync()
            tb = time.perf_counter()
            u, st = b.gaussian_beams(grid, omegas, eps, fan_size=M, cutoff=cutoff, max_width=max_width, edge_taper=edge_taper,
                                     stats=True)
        finally:
            b.close()
        tc = time.perf_counter()
        tot["groups"] += 1
        tot["trace_ms"] += (tb - ta) * 1e3
        tot["beam_ms"] += (tc - tb) * 1e3
        for k in ("segments", "tile_entries", "pairs_tested", "pairs_inside", "capped", "prep_ms", "bin_ms", "gather_ms"):
            tot[k] = tot.get(k, 0) + st[k]
        if res is None:
            res = np.empty((S,) + u.shape[1:], dtype=u.dtype)
        res[g0:g0 + len(sg)] = u
    return (res, tot) if stats else res


def kirchhoff_stats(st):
    """aux_ms: on an anti-aliased handle the part of kernel_ms that is not the pair kernel (the bank's filter in migrate, the sum
    over the levels in model); 0 elsewhere"""
    return {"kernel_ms": st.kernel_ms, "upload_ms": st.upload_ms, "pairs": int(st.pairs), "contributing": int(st.contributing),
            "scale_exp": int(st.scale_exp), "aux_ms": st.reserved[0] * 1e-6}


ANTIALIAS_DEFAULTS = dict(hw=(0, 1, 2, 4, 8), asrc=0.0, arec=0.0, amid=0.0)


def position_slope(tab, n_at_positions, direction=(1.0, 0.0)):
    """pt of T's shape for Kirchhoff(..., pt=): the derivative of the table's traveltimes with respect to the surface position along
    the line of unit `direction`, by reciprocity -n(p) (cos theta0 e_x + sin theta0 e_y) from the table's launch angles theta0
    (traveltime_table's column).  n_at_positions [P]: the refractive index at each position (Field.n_gradient(x, y)[0]).  NaN
    where the table has no arrival."""
    th = np.asarray(tab["theta0"], dtype=np.float64)
    n = np.asarray(n_at_positions, dtype=np.float64).reshape(-1)
    if n.shape[0] != th.shape[0]:
        raise ValueError("position_slope: n_at_positions must have one value per position")
    ex, ey = float(direction[0]), float(direction[1])
    n = n.reshape((-1,) + (1,) * (th.ndim - 1))
    return -n * (np.cos(th) * ex + np.sin(th) * ey)


def hilbert(d):
    """The Hilbert transform along the last axis, H[cos] = sin: the imaginary part of scipy.signal.hilbert's analytic signal, by
    numpy.fft with scipy's mask (DC and Nyquist zeroed, positive frequencies doubled).  Circular: the transform wraps around the
    ends of the axis, so the caller pads a trace whose energy reaches them.  As a matrix it is a real antisymmetric circulant:
    the transpose is -H up to rounding."""
    d = np.asarray(d, dtype=np.float64)
    n = d.shape[-1]
    h = np.zeros(n)
    if n % 2 == 0:
        h[1:n // 2] = 2.0
    else:
        h[1:(n + 1) // 2] = 2.0
    return np.fft.ifft(np.fft.fft(d, axis=-1) * h, axis=-1).imag


def hilbert_taps(n):
    """rtmi_hilbert_taps: the taps c_1 .. c_K, K = (n - 1) // 2, of the time-domain form of `hilbert` that the device evaluates
    (Kirchhoff.hilbert; include/rtmi.h has the formula).  Host only: no device is touched."""
    n = int(n)
    K = max((n - 1) // 2, 0)
    taps = np.zeros(max(K, 1))                     # n = 1 and n = 2 have no taps: nothing is written
    check(lib().rtmi_hilbert_taps(n, dptr(taps)))
    return taps[:K]


def debug_hilbert(x, add=None, negate=False):
    """rtmi_debug_hilbert: Kirchhoff.hilbert_device's kernel on host arrays [N, nt] without a handle -> (add or +0) +- H x"""
    xx = np.ascontiguousarray(x, dtype=np.float64)
    if xx.ndim != 2:
        raise ValueError("debug_hilbert: x must be [N, nt]")
    aa = None if add is None else np.ascontiguousarray(add, dtype=np.float64)
    if aa is not None and aa.shape != xx.shape:
        raise ValueError("debug_hilbert: add must have x's shape")
    y = np.empty_like(xx)
    check(lib().rtmi_debug_hilbert(dptr(xx), xx.shape[0], xx.shape[1], dptr(aa), 1 if negate else 0, dptr(y)))
    return y


def half_derivative_taps(L, dt):
    """rtmi_half_derivative_taps: L causal taps (origin 0) of the 2-D half-derivative sqrt(i w), the pi/4 filter, at the sample
    interval dt: g_0 = 1, g_k = g_(k-1) (2 k - 3) / (2 k), each times 1 / sqrt(dt) (include/rtmi.h).  Host only: no device is
    touched.  The filter of Kirchhoff.set_filter is usually this convolved with the wavelet:
      ricker = ...                                                    # 2 M + 1 zero-phase taps, its centre at index M
      op.set_filter(np.convolve(ricker, half_derivative_taps(L, dt)), origin=M)"""
    L = int(L)
    taps = np.zeros(max(L, 1))
    check(lib().rtmi_half_derivative_taps(L, float(dt), dptr(taps)))
    return taps[:L]


def illumination_scale(illum, eps=1e-3):
    """The column scale of an illumination map: 1 / sqrt(illum + eps max(illum)), and 0 (a masked value) where illum is 0"""
    ill = np.asarray(illum, dtype=np.float64)
    top = float(ill.max()) if ill.size else 0.0
    out = np.zeros_like(ill)
    lit = ill > 0.0
    out[lit] = 1.0 / np.sqrt(ill[lit] + float(eps) * top)
    return out


def _lsqr_options(who, per, nm, row_weight, col_scale, x0):
    """-> (rtmi_lsqr_options, the arrays it points into, which the caller keeps alive over the call)"""
    lo = _lib.LsqrOptions()
    keep = []
    for field, a, n in (("row_weight", row_weight, per), ("col_scale", col_scale, nm), ("x0", x0, nm)):
        if a is None:
            continue
        aa = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        if aa.size != n:
            raise ValueError(f"{who}: {field} must have {n} values")
        keep.append(aa)
        setattr(lo, field, dptr(aa))
    return lo, keep


class Kirchhoff:
    """Kirchhoff migration and modelling from traveltime tables (rtmi_kirchhoff_*, include/rtmi.h).  T [P, ny, nx]:
    traveltime_table's T for P surface positions; isrc, irec [N]: each trace's source and receiver position in [0, P); nt samples
    per trace at t0 + j dt; amp, theta [P, ny, nx] and weights [N] optional; nbin > 0 splits the image into opening-angle bins of
    width dopen (needs theta).  The tables stay on the device until close().
      migrate(data [N, nt]) -> image [nb, ny, nx] ([ny, nx] when nbin == 0), defined bit for bit by the trace order
      model(m)              -> data [N, nt], the transpose; the same bits in every trace order
      as_linear_operator()  scipy LinearOperator of shape (N nt, nb ny nx): matvec = model, rmatvec = migrate
    With stats=True the calls return (result, stats).
    A 4-D T [P, K, ny, nx] (traveltime_table(arrivals=K)'s layout; amp, theta and the optional kmah of that shape) makes a handle
    over all K^2 pairs of a source and a receiver arrival, each rotated by its caustic phase (rtmi_kirchhoff_create_multi):
      migrate_channels(d0, d1) -> image    and    model_channels(m) -> (ch0, ch1)
    are the bit-defined transposes between the model and the two trace channels (d1 may be None, and ch1 is zeros, without kmah);
    the full trace is ch0 + H ch1 with H = hilbert (circular: pad the traces), so on such a handle
      model(m) = ch0 + hilbert(ch1)    and    migrate(d) = migrate_channels(d, -hilbert(d)),   its transpose since H^T = -H.
    With pt (of T's shape: dT/d(position), position_slope) the pair is anti-aliased by operator slope (rtmi_kirchhoff_create_aa,
    DESIGN.md 20): antialias = dict(hw=(0, 1, 2, 4, 8), asrc=0.0, arec=0.0, amid=0.0), the triangle half-widths of the levels in
    samples and the trace spacing along the source, receiver and midpoint axes (keys left out take these defaults).  A 3-D T is
    then taken as K = 1; every call above works unchanged, and aa_filter(d) returns the bank [nlev, N, nt] of one channel.
    On the device, for every kind of handle:
      migrate_device(d0, d1=None) -> image    and    model_device(m) -> data, or (ch0, ch1) on a handle with kmah
    take and return fp64 contiguous torch tensors on the handle's device: the bits of the calls above, no copy through the host.
      lsqr(d, iter_lim, damp=0.0, atol=0.0, btol=0.0) -> dict(x, istop, itn, r1norm, r2norm, anorm, arnorm)
    is least-squares migration by LSQR in scipy's operation order with every vector on the device (rtmi_kirchhoff_lsqr): the data
    go up once and x comes down once; defined bit for bit.  The library refuses a handle with kmah, unless hilbert="device":
    then the solver is rtmi_kirchhoff_lsqr_full, for the full trace ch0 + H ch1 with H on the device:
      hilbert(d) -> H d on host arrays    and    hilbert_device(x, add=None, negate=False) -> (add or +0) +- H x on torch tensors
    are that H, on every kind of handle, for nt <= 16384: the matrix of `hilbert` evaluated in the time domain and defined bit for
    bit, its transpose -H in every bit.  model, migrate and as_linear_operator() keep the FFT form and their bits.
    The wavelet and the 2-D half-derivative on the device:
      set_filter(taps, origin=0)    keeps taps f[0 .. L), L <= 2048, on the handle (None clears); tap `origin` is lag zero
      filter(d, transpose=False) -> F d or F^T d on host arrays    and    filter_device(x, transpose=False) on torch tensors
    are the linear convolution (F d)[i] = sum_k f[k] d[i - k + origin] along the traces, zero outside them, and its exact
    transpose, defined bit for bit; the usual taps are np.convolve(ricker, half_derivative_taps(L, dt)) with origin at the
    Ricker's centre.  lsqr(..., filtered=True) solves with that filter inside the operator, F (ch0 + H ch1), and its exact
    transpose (rtmi_kirchhoff_lsqr_filtered).  Every other call ignores a set filter."""

    def __init__(self, T, isrc, irec, nt, dt, t0=0.0, amp=None, theta=None, weights=None, nbin=0, dopen=None, kmah=None, pt=None,
                 antialias=None):
        T = np.ascontiguousarray(T, dtype=np.float64)
        if T.ndim not in (3, 4):
            raise ValueError("Kirchhoff: T must be [P, ny, nx] or [P, K, ny, nx]")
        if antialias is not None and pt is None:
            raise ValueError("Kirchhoff: antialias needs pt")
        self.karr = T.shape[1] if T.ndim == 4 else 0
        if kmah is not None and not self.karr:
            raise ValueError("Kirchhoff: kmah needs T [P, K, ny, nx]")
        P, ny, nx = T.shape[0], T.shape[-2], T.shape[-1]
        opt = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (amp, theta, kmah, pt)]
        for a, name in zip(opt, ("amp", "theta", "kmah", "pt")):
            if a is not None and a.shape != T.shape:
                raise ValueError(f"Kirchhoff: {name} must have T's shape")
        si = np.ascontiguousarray(isrc, dtype=np.int32).reshape(-1)
        ri = np.ascontiguousarray(irec, dtype=np.int32).reshape(-1)
        if si.shape != ri.shape:
            raise ValueError("Kirchhoff: isrc and irec must have one length")
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w is not None and w.shape != si.shape:
            raise ValueError("Kirchhoff: weights must have isrc's length")
        self.antialias = None
        if pt is not None:
            unknown = set(antialias or {}) - set(ANTIALIAS_DEFAULTS)
            if unknown:
                raise ValueError(f"Kirchhoff: antialias has unknown keys {sorted(unknown)}")
            self.antialias = dict(ANTIALIAS_DEFAULTS, **(antialias or {}))
            self.antialias["hw"] = tuple(int(v) for v in self.antialias["hw"])
            if len(self.antialias["hw"]) > _lib.KIRCHHOFF_MAX_LEVELS:
                raise ValueError("Kirchhoff: antialias hw has more than 8 levels")
            self.karr = self.karr or 1                 # a 3-D table is the K = 1 layout
        kp = _lib.KirchhoffAAParams() if pt is not None else _lib.KirchhoffMultiParams() if self.karr else _lib.KirchhoffParams()
        kp.nx, kp.ny, kp.P, kp.N, kp.nt = nx, ny, P, len(si), int(nt)
        kp.t0 = float(t0); kp.dt = float(dt); kp.nbin = int(nbin); kp.dopen = float(dopen or 0.0)
        self.N, self.nt, self.nb, self.nbin, self.ny, self.nx = len(si), int(nt), max(int(nbin), 1), int(nbin), ny, nx
        self.shape = (self.N * self.nt, self.nb * ny * nx)
        self.has_kmah = kmah is not None
        self._h = None
        self._filter = None                            # (L, origin) of set_filter, None with no filter set
        h = C.c_void_p()
        if pt is not None:
            aa = self.antialias
            kp.karr = self.karr
            kp.nlev = len(aa["hw"])
            for i, v in enumerate(aa["hw"]):
                kp.hw[i] = v
            kp.asrc, kp.arec, kp.amid = float(aa["asrc"]), float(aa["arec"]), float(aa["amid"])
            self.nlev = kp.nlev
            check(lib().rtmi_kirchhoff_create_aa(C.byref(kp), dptr(T), dptr(opt[0]), dptr(opt[1]), dptr(opt[2]), dptr(opt[3]),
                                                 si.ctypes.data_as(_lib._ip), ri.ctypes.data_as(_lib._ip), dptr(w), C.byref(h)))
        elif self.karr:
            kp.karr = self.karr
            check(lib().rtmi_kirchhoff_create_multi(C.byref(kp), dptr(T), dptr(opt[0]), dptr(opt[1]), dptr(opt[2]),
                                                    si.ctypes.data_as(_lib._ip), ri.ctypes.data_as(_lib._ip), dptr(w), C.byref(h)))
        else:
            check(lib().rtmi_kirchhoff_create(C.byref(kp), dptr(T), dptr(opt[0]), dptr(opt[1]), si.ctypes.data_as(_lib._ip),
                                              ri.ctypes.data_as(_lib._ip), dptr(w), C.byref(h)))
        self._h = h

    @classmethod
    def from_table(cls, tab, isrc, irec, nt, dt, t0=0.0, amplitude=False, weights=None, nbin=0, dopen=None, antialias=None):
        """From traveltime_table's dict: its T, its theta when nbin > 0, and its G as amp when amplitude is asked for; with
        arrivals=K tables (a 4-D T) also its kmah whenever the dict has one.  antialias: Kirchhoff's dict with two more keys,
        n_at_positions [P] and optionally direction, from which position_slope takes pt off the table's theta0."""
        multi = np.ndim(tab["T"]) == 4
        pt = None
        if antialias is not None:
            antialias = dict(antialias)
            if "n_at_positions" not in antialias:
                raise ValueError("Kirchhoff.from_table: antialias needs n_at_positions")
            pt = position_slope(tab, antialias.pop("n_at_positions"), antialias.pop("direction", (1.0, 0.0)))
        return cls(tab["T"], isrc, irec, nt, dt, t0=t0, amp=tab["G"] if amplitude else None,
                   theta=tab["theta"] if nbin else None, weights=weights, nbin=nbin, dopen=dopen,
                   kmah=tab["kmah"] if multi and "kmah" in tab else None, pt=pt, antialias=antialias)

    def _open(self):
        if not self._h:
            raise RuntimeError("Kirchhoff: the handle is closed")
        return self._h

    def migrate(self, data, stats=False):
        if self.karr:
            d = np.ascontiguousarray(data, dtype=np.float64).reshape(self.N, self.nt)
            return self.migrate_channels(d, -hilbert(d) if self.has_kmah else None, stats=stats)
        d = np.ascontiguousarray(data, dtype=np.float64)
        if d.size != self.N * self.nt:
            raise ValueError("Kirchhoff.migrate: data must be [N, nt]")
        img = np.empty((self.nb, self.ny, self.nx))
        st = _lib.KirchhoffStats()
        check(lib().rtmi_kirchhoff_migrate(self._open(), dptr(d), dptr(img), C.byref(st)))
        if self.nbin == 0:
            img = img[0]
        return (img, kirchhoff_stats(st)) if stats else img

    def model(self, m, stats=False):
        if self.karr:
            (c0, c1), st = self.model_channels(m, stats=True)
            d = c0 + hilbert(c1) if self.has_kmah else c0
            return (d, st) if stats else d
        mm = np.ascontiguousarray(m, dtype=np.float64)
        if mm.size != self.nb * self.ny * self.nx:
            raise ValueError("Kirchhoff.model: m must be [nb, ny, nx]")
        d = np.empty((self.N, self.nt))
        st = _lib.KirchhoffStats()
        check(lib().rtmi_kirchhoff_model(self._open(), dptr(mm), dptr(d), C.byref(st)))
        return (d, kirchhoff_stats(st)) if stats else d

    def _multi(self, who):
        if not self.karr:
            raise ValueError(f"Kirchhoff.{who}: the handle has one arrival per node (T [P, ny, nx]); use migrate / model")

    def migrate_channels(self, d0, d1=None, stats=False):
        """rtmi_kirchhoff_migrate2: (channel 0, channel 1) [N, nt] each -> image; d1 may be None only without kmah"""
        self._multi("migrate_channels")
        d = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (d0, d1)]
        if any(a is not None and a.size != self.N * self.nt for a in d) or d[0] is None:
            raise ValueError("Kirchhoff.migrate_channels: each channel must be [N, nt]")
        img = np.empty((self.nb, self.ny, self.nx))
        st = _lib.KirchhoffStats()
        check(lib().rtmi_kirchhoff_migrate2(self._open(), dptr(d[0]), dptr(d[1]), dptr(img), C.byref(st)))
        if self.nbin == 0:
            img = img[0]
        return (img, kirchhoff_stats(st)) if stats else img

    def model_channels(self, m, stats=False):
        """rtmi_kirchhoff_model2: m -> (channel 0, channel 1), [N, nt] each; channel 1 is zeros without kmah"""
        self._multi("model_channels")
        mm = np.ascontiguousarray(m, dtype=np.float64)
        if mm.size != self.nb * self.ny * self.nx:
            raise ValueError("Kirchhoff.model_channels: m must be [nb, ny, nx]")
        d0 = np.empty((self.N, self.nt)); d1 = np.empty((self.N, self.nt))
        st = _lib.KirchhoffStats()
        check(lib().rtmi_kirchhoff_model2(self._open(), dptr(mm), dptr(d0), dptr(d1), C.byref(st)))
        return ((d0, d1), kirchhoff_stats(st)) if stats else (d0, d1)

    def aa_filter(self, d):
        """rtmi_kirchhoff_aa_filter: one channel [N, nt] -> its bank [nlev, N, nt], level l the triangle of half-width hw[l]"""
        if self.antialias is None:
            raise ValueError("Kirchhoff.aa_filter: the handle has no pt (antialias)")
        dd = np.ascontiguousarray(d, dtype=np.float64)
        if dd.size != self.N * self.nt:
            raise ValueError("Kirchhoff.aa_filter: d must be [N, nt]")
        bank = np.empty((self.nlev, self.N, self.nt))
        check(lib().rtmi_kirchhoff_aa_filter(self._open(), dptr(dd), dptr(bank)))
        return bank

    def _device_tensor(self, who, t, name, size):
        import torch
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"Kirchhoff.{who}: {name} must be a torch tensor")
        if t.dtype != torch.float64:
            raise TypeError(f"Kirchhoff.{who}: {name} must be float64")
        if t.numel() != size:
            raise ValueError(f"Kirchhoff.{who}: {name} must have {size} values")
        if not t.is_contiguous():
            raise ValueError(f"Kirchhoff.{who}: {name} must be contiguous")
        return t

    def _on_device(self, who, **tensors):
        for name, t in tensors.items():
            if t is not None and not t.is_cuda:       # which GPU it is on, the library checks against the handle's
                raise ValueError(f"Kirchhoff.{who}: {name} must be a tensor on a GPU, not on the host")

    def migrate_device(self, d0, d1=None, stats=False):
        """rtmi_kirchhoff_migrate_dev: channel 0 and, on a handle with kmah, channel 1 [N, nt] -> image, torch tensors on the
        handle's device"""
        import torch
        who = "migrate_device"
        self._device_tensor(who, d0, "d0", self.N * self.nt)
        if d1 is not None:
            self._device_tensor(who, d1, "d1", self.N * self.nt)
        elif self.has_kmah:
            raise ValueError("Kirchhoff.migrate_device: a handle with kmah needs d1")
        self._on_device(who, d0=d0, d1=d1)
        h = self._open()
        img = torch.empty((self.nb, self.ny, self.nx), dtype=torch.float64, device=d0.device)
        st = _lib.KirchhoffStats()
        torch.cuda.synchronize(d0.device)              # the library works on the null stream
        check(lib().rtmi_kirchhoff_migrate_dev(h, d0.data_ptr(), None if d1 is None else d1.data_ptr(), img.data_ptr(), C.byref(st)))
        if self.nbin == 0:
            img = img[0]
        return (img, kirchhoff_stats(st)) if stats else img

    def model_device(self, m, stats=False):
        """rtmi_kirchhoff_model_dev: m [nb, ny, nx] -> data [N, nt], or (ch0, ch1) on a handle with kmah; torch tensors on the
        handle's device"""
        import torch
        self._device_tensor("model_device", m, "m", self.nb * self.ny * self.nx)
        self._on_device("model_device", m=m)
        h = self._open()
        d0 = torch.empty((self.N, self.nt), dtype=torch.float64, device=m.device)
        d1 = torch.empty((self.N, self.nt), dtype=torch.float64, device=m.device) if self.has_kmah else None
        st = _lib.KirchhoffStats()
        torch.cuda.synchronize(m.device)
        check(lib().rtmi_kirchhoff_model_dev(h, m.data_ptr(), d0.data_ptr(), None if d1 is None else d1.data_ptr(), C.byref(st)))
        out = (d0, d1) if self.has_kmah else d0
        return (out, kirchhoff_stats(st)) if stats else out

    def hilbert(self, d):
        """rtmi_kirchhoff_hilbert: H d along the last axis of [N, nt] host arrays, evaluated on the device in the time domain"""
        dd = np.ascontiguousarray(d, dtype=np.float64)
        if dd.size != self.N * self.nt:
            raise ValueError("Kirchhoff.hilbert: d must be [N, nt]")
        y = np.empty((self.N, self.nt))
        check(lib().rtmi_kirchhoff_hilbert(self._open(), dptr(dd), dptr(y)))
        return y

    def hilbert_device(self, x, add=None, negate=False):
        """rtmi_kirchhoff_hilbert_dev: (add or +0) + H x, or - H x with negate, [N, nt] torch tensors on the handle's device.  With
        add the result is written over add and add is returned; x is never written."""
        import torch
        who = "hilbert_device"
        self._device_tensor(who, x, "x", self.N * self.nt)
        if add is not None:
            self._device_tensor(who, add, "add", self.N * self.nt)
        self._on_device(who, x=x, add=add)
        if add is not None and add.data_ptr() == x.data_ptr():
            raise ValueError("Kirchhoff.hilbert_device: add may not be x")
        h = self._open()
        y = add if add is not None else torch.empty((self.N, self.nt), dtype=torch.float64, device=x.device)
        torch.cuda.synchronize(x.device)               # the library works on the null stream
        check(lib().rtmi_kirchhoff_hilbert_dev(h, x.data_ptr(), None if add is None else add.data_ptr(), 1 if negate else 0, y.data_ptr()))
        return y

    def set_filter(self, taps, origin=0):
        """rtmi_kirchhoff_set_filter: keep the taps f[0 .. L), 1 <= L <= 2048, finite, on the handle's device; tap `origin` is
        lag zero (0: causal; M for a zero-phase wavelet of 2 M + 1 taps).  None clears the filter.  A second call replaces the
        first.  The usual composition: set_filter(np.convolve(ricker, half_derivative_taps(L, dt)), origin=M), M the index of
        the Ricker's centre."""
        if taps is None:
            check(lib().rtmi_kirchhoff_set_filter(self._open(), None, 0, 0))
            self._filter = None
            return
        f = np.ascontiguousarray(taps, dtype=np.float64)
        if f.ndim != 1 or f.size < 1:
            raise ValueError("Kirchhoff.set_filter: taps must be a vector of at least one value (None clears the filter)")
        check(lib().rtmi_kirchhoff_set_filter(self._open(), dptr(f), f.size, int(origin)))    # the library checks the rest
        self._filter = (int(f.size), int(origin))

    def filter(self, d, transpose=False):
        """rtmi_kirchhoff_filter: F d, or F^T d with transpose, along the last axis of [N, nt] host arrays, on the device"""
        dd = np.ascontiguousarray(d, dtype=np.float64)
        if dd.size != self.N * self.nt:
            raise ValueError("Kirchhoff.filter: d must be [N, nt]")
        y = np.empty((self.N, self.nt))
        check(lib().rtmi_kirchhoff_filter(self._open(), dptr(dd), 1 if transpose else 0, dptr(y)))
        return y

    def filter_device(self, x, transpose=False):
        """rtmi_kirchhoff_filter_dev: F x, or F^T x with transpose, [N, nt] torch tensors on the handle's device; x is never
        written, the result is a new tensor"""
        import torch
        who = "filter_device"
        self._device_tensor(who, x, "x", self.N * self.nt)
        self._on_device(who, x=x)
        h = self._open()
        y = torch.empty((self.N, self.nt), dtype=torch.float64, device=x.device)
        torch.cuda.synchronize(x.device)               # the library works on the null stream
        check(lib().rtmi_kirchhoff_filter_dev(h, x.data_ptr(), 1 if transpose else 0, y.data_ptr()))
        return y

    def illumination(self, stats=False):
        """rtmi_kirchhoff_illumination: per image value the sum over migrate's contributing pairs of c^2 ((1 - a)^2 + a^2), shaped
        like migrate's image; diag(L^T L) exactly on a handle with one arrival and no anti-alias levels, else that diagonal
        without the cross terms, the level filters, H and F"""
        ill = np.empty((self.nb, self.ny, self.nx))
        st = _lib.KirchhoffStats()
        check(lib().rtmi_kirchhoff_illumination(self._open(), dptr(ill), C.byref(st)))
        if self.nbin == 0:
            ill = ill[0]
        return (ill, kirchhoff_stats(st)) if stats else ill

    def illumination_device(self, stats=False):
        """rtmi_kirchhoff_illumination_dev: illumination() into a new torch tensor on the current GPU, which must be the handle's"""
        import torch
        h = self._open()
        ill = torch.empty((self.nb, self.ny, self.nx), dtype=torch.float64, device="cuda")
        st = _lib.KirchhoffStats()
        torch.cuda.synchronize(ill.device)             # the library works on the null stream
        check(lib().rtmi_kirchhoff_illumination_dev(h, ill.data_ptr(), C.byref(st)))
        if self.nbin == 0:
            ill = ill[0]
        return (ill, kirchhoff_stats(st)) if stats else ill

    def lsqr(self, d, iter_lim, damp=0.0, atol=0.0, btol=0.0, history=False, stats=False, hilbert=None, filtered=False,
             row_weight=None, col_scale=None, x0=None, eps=1e-3):
        """rtmi_kirchhoff_lsqr: min |L x - d|^2 + damp^2 |x|^2 from x = 0, every vector on the device.  -> dict: x shaped like
        migrate's image, istop (scipy's 0, 1, 2, 7; _lib.LSQR_RANGE: a norm left fp64's normal range), itn, r1norm, r2norm, anorm,
        arnorm; with history=True also history [itn, 4] (alfa, beta, r1norm, arnorm after each iteration); with stats=True also
        stats (total_ms, operator_ms, vector_ms, bytes_device).  hilbert="device": rtmi_kirchhoff_lsqr_full, which on a handle
        with kmah solves for the full trace ch0 + H ch1 (model's trace, with the device's H) and on any other handle is the same
        call; None: a handle with kmah is refused.  filtered=True: rtmi_kirchhoff_lsqr_filtered, the same with set_filter's F
        inside the operator, A = F (ch0 + H ch1) and its exact transpose; it needs a filter, and on a handle with kmah
        hilbert="device".
        row_weight [N, nt], col_scale and x0 shaped like the image: rtmi_kirchhoff_lsqr_weighted, min |W L D y - W (d - L x0)|^2 +
        damp^2 |y|^2 and x = x0 + D y, with the operator hilbert= / filtered= choose; a col_scale of 0 masks a value, which comes
        back as x0's.  col_scale="illumination": 1 / sqrt(illum + eps max(illum)) of illumination(), 0 where illum is 0.  Without
        these keywords the call is the one it was."""
        if hilbert not in (None, "device"):
            raise ValueError('Kirchhoff.lsqr: hilbert must be None or "device"')
        if filtered:
            if getattr(self, "_filter", None) is None:
                raise ValueError("Kirchhoff.lsqr: filtered=True needs a filter (set_filter)")
            if hilbert is None and self.has_kmah:
                raise ValueError('Kirchhoff.lsqr: filtered=True on a handle with kmah needs hilbert="device": the filtered trace is '
                                 "F (ch0 + H ch1)")
        dd = np.ascontiguousarray(d, dtype=np.float64)
        if dd.size != self.N * self.nt:
            raise ValueError("Kirchhoff.lsqr: d must be [N, nt]")
        iter_lim = int(iter_lim)
        if iter_lim < 1:
            raise ValueError("Kirchhoff.lsqr: iter_lim must be >= 1")
        lp = _lib.LsqrParams()
        lp.iter_lim, lp.damp, lp.atol, lp.btol = iter_lim, float(damp), float(atol), float(btol)
        x = np.empty((self.nb, self.ny, self.nx))
        hist = np.zeros((iter_lim, 4)) if history else None
        st = _lib.LsqrStats()
        if row_weight is None and col_scale is None and x0 is None:
            solver = (lib().rtmi_kirchhoff_lsqr_filtered if filtered else
                      lib().rtmi_kirchhoff_lsqr_full if hilbert == "device" else lib().rtmi_kirchhoff_lsqr)
            check(solver(self._open(), C.byref(lp), dptr(dd), dptr(x), dptr(hist), C.byref(st)))
        else:
            if isinstance(col_scale, str):
                if col_scale != "illumination":
                    raise ValueError('Kirchhoff.lsqr: col_scale must be an array or "illumination"')
                col_scale = illumination_scale(self.illumination(), eps)
            lo, keep = _lsqr_options("Kirchhoff.lsqr", self.N * self.nt, self.nb * self.ny * self.nx, row_weight, col_scale, x0)
            op = _lib.LSQR_OP_FILTERED if filtered else _lib.LSQR_OP_FULL if hilbert == "device" else _lib.LSQR_OP_PLAIN
            check(lib().rtmi_kirchhoff_lsqr_weighted(self._open(), C.byref(lp), C.byref(lo), op, dptr(dd), dptr(x), dptr(hist), C.byref(st)))
        out = {"x": x if self.nbin else x[0], "istop": int(st.istop), "itn": int(st.itn), "r1norm": st.r1norm, "r2norm": st.r2norm,
               "anorm": st.anorm, "arnorm": st.arnorm}
        if history:
            out["history"] = hist[:st.itn].copy()
        if stats:
            out["stats"] = {"total_ms": st.total_ms, "operator_ms": st.operator_ms, "vector_ms": st.vector_ms,
                            "bytes_device": int(st.bytes_device)}
        return out

    def as_linear_operator(self):
        from scipy.sparse.linalg import LinearOperator
        return LinearOperator(self.shape, matvec=lambda m: self.model(m).reshape(-1),
                              rmatvec=lambda d: self.migrate(d).reshape(-1), dtype=np.float64)

    def close(self):
        if self._h:
            lib().rtmi_kirchhoff_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def locate_stats(st):
    return {"kernel_ms": st.kernel_ms, "upload_ms": st.upload_ms, "triples": int(st.triples), "contributing": int(st.contributing),
            "search_ms": st.reserved[0] * 1e-6}                   # k_locate's own part of kernel_ms


def edt_stats(st):
    return {"kernel_ms": st.kernel_ms, "upload_ms": st.upload_ms, "triples": int(st.triples), "contributing": int(st.contributing),
            "search_ms": st.reserved[0] * 1e-6,                    # k_edt's own part of kernel_ms
            "groups": int(st.reserved[1])}                         # the groups of event chunks the call was walked in


def pdf_stats(st):
    return {"kernel_ms": st.kernel_ms, "upload_ms": st.upload_ms, "triples": int(st.triples), "contributing": int(st.contributing),
            "search_ms": st.reserved[0] * 1e-6,                    # the search kernel's own part of kernel_ms
            "groups": int(st.reserved[1]),                         # the groups of events the call was walked in
            "pdf_ms": st.reserved[2] * 1e-6}                       # the pdf kernels' part of kernel_ms


def edt_exp(z):
    """rtmi_edt_exp: exp(z) for z in [-700, 0] as rtmi_locate_edt's device code evaluates it (numpy's array exp, restated), on the
    host; tests/edt_ref.py takes its exp from here"""
    zz = np.ascontiguousarray(z, dtype=np.float64)
    out = np.empty_like(zz)
    check(lib().rtmi_edt_exp(dptr(zz.reshape(-1)), dptr(out.reshape(-1)), zz.size))
    return out


def stack_stats(st):
    return {"kernel_ms": st.kernel_ms, "upload_ms": st.upload_ms, "triples": int(st.triples), "contributing": int(st.contributing),
            "truncated": bool(st.truncated), "search_ms": st.reserved[0] * 1e-6,            # k_stack's own part of kernel_ms
            "parts": int(st.reserved[1])}                                                   # the parts the scan was split into


class Locator:
    """Event location by grid search over traveltime tables (rtmi_locator_*, rtmi_locate, include/rtmi.h).
    T [P, ny, nx]: one table per station on grid = (gx0, gdx, nx, gy0, gdy, ny), traveltime_table's T with the stations as its
    sources (reciprocity); the tables stay on the device until close().
      locate(picks [E, P], weights=None, min_picks=None, maps=False, refine=True, stats=False) -> dict of arrays over the events:
        x, y, t0         the location and origin time: the quadratic refinement through the 3 x 3 window where it is accepted
                         (refined = 1), the best node's own otherwise, and always with refine=False
        node, ix, iy     the best node (-1: no node has enough picks); count, obj, rms = sqrt(obj), sw there
        cov [E, 2, 2]    the covariance of (x, y) of a refined event, NaN otherwise
        win_obj, win_tau [E, 3, 3], dx, dy, t0_node, ref; with maps=True also maps [E, ny, nx], obj at every node
      NaN in picks: no pick; weights [E, P] (1 / sigma^2; 0, negative and non-finite ones drop the pick); min_picks, an int or
      [E]: the fewest contributing picks of a node (default: all the event's valid picks).
      locate_device(picks, weights=None, min_picks=None, maps=False, ...) takes torch tensors on the handle's device (fp64 picks
      and weights, int32 min_picks) and returns maps as a tensor on it: the same bits, no copy of them through the host.
      locate_edt(picks, sigma, ...) is the robust search by equal differential time, for picks that may contain outliers
      (see its own text); locate_edt_device its form on torch tensors.
      pdf(picks, sigma, method="l2" | "edt", ...) is either search with the pdf of its whole map: expectation, covariance,
      confidence regions, marginals and samples (see its own text); pdf_device its form on torch tensors.
      stack(traces [P, nt], dt, t0, scan=(o0, od, M), ...) needs no picks: it stacks one characteristic function per station along
      every node's moveout for every origin time of the scan and takes events from the peaks (see stack's own text).
    With stats=True the calls return (result, stats)."""

    def __init__(self, T, grid):
        T = np.ascontiguousarray(T, dtype=np.float64)
        if T.ndim != 3:
            raise ValueError("Locator: T must be [P, ny, nx]")
        gx0, gdx, nx, gy0, gdy, ny = grid
        if T.shape[1:] != (int(ny), int(nx)):
            raise ValueError("Locator: T must be [P, ny, nx] of the grid")
        lp = _lib.LocatorParams()
        lp.nx, lp.ny, lp.P = int(nx), int(ny), T.shape[0]
        lp.gx0, lp.gdx, lp.gy0, lp.gdy = float(gx0), float(gdx), float(gy0), float(gdy)
        self.P, self.ny, self.nx, self.grid = T.shape[0], int(ny), int(nx), tuple(grid)
        self._h = None
        h = C.c_void_p()
        check(lib().rtmi_locator_create(C.byref(lp), dptr(T), C.byref(h)))
        self._h = h

    @classmethod
    def from_table(cls, tab, grid):
        """From traveltime_table's dict: its T [S, ny, nx], or slot 0 (the first arrival) of a T [S, K, ny, nx]"""
        T = np.asarray(tab["T"])
        return cls(T[:, 0] if T.ndim == 4 else T, grid)

    def _open(self):
        if not self._h:
            raise RuntimeError("Locator: the handle is closed")
        return self._h

    def _result(self, res, E, refine):
        a = np.frombuffer(res, dtype=np.dtype(_lib.LocateResult)).copy() if E else np.zeros(0, dtype=np.dtype(_lib.LocateResult))
        out = {"node": a["node"].copy(), "ix": a["ix"].copy(), "iy": a["iy"].copy(), "count": a["n"].copy(), "sw": a["sw"].copy(),
               "obj": a["obj"].copy(), "ref": a["ref"].copy(), "t0_node": a["t0"].copy(),
               "win_obj": a["win_obj"].reshape(E, 3, 3).copy(), "win_tau": a["win_tau"].reshape(E, 3, 3).copy()}
        with np.errstate(invalid="ignore"):
            out["rms"] = np.sqrt(out["obj"])
        cov = np.full((E, 2, 2), np.nan)
        if refine:
            out.update(x=a["x"].copy(), y=a["y"].copy(), t0=a["t0_refined"].copy(), dx=a["dx"].copy(), dy=a["dy"].copy(),
                       refined=a["refined"].copy())
            c = a["cov"].reshape(E, 3)
            cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 0], cov[:, 1, 1] = c[:, 0], c[:, 1], c[:, 1], c[:, 2]
        else:
            gx0, gdx, _, gy0, gdy, _ = self.grid
            none = out["node"] < 0
            out.update(x=np.where(none, np.nan, float(gx0) + out["ix"] * float(gdx)), y=np.where(none, np.nan, float(gy0) + out["iy"] * float(gdy)),
                       t0=out["t0_node"].copy(), dx=np.where(none, np.nan, 0.0), dy=np.where(none, np.nan, 0.0),
                       refined=np.zeros(E, dtype=np.int32))
        out["cov"] = cov
        return out

    def locate(self, picks, weights=None, min_picks=None, maps=False, refine=True, stats=False):
        t = np.ascontiguousarray(picks, dtype=np.float64)
        if t.ndim != 2 or t.shape[1] != self.P:
            raise ValueError(f"Locator.locate: picks must be [E, {self.P}]")
        E = t.shape[0]
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        if w is not None and w.shape != t.shape:
            raise ValueError("Locator.locate: weights must have the shape of picks")
        need = None
        if min_picks is not None:
            need = np.ascontiguousarray(np.broadcast_to(np.asarray(min_picks, dtype=np.int32), (E,)))
        h = self._open()
        res = (_lib.LocateResult * E)()
        m = np.empty((E, self.ny, self.nx)) if maps else None
        st = _lib.LocateStats()
        check(lib().rtmi_locate(h, E, dptr(t), dptr(w), None if need is None else need.ctypes.data_as(_lib._ip), res, dptr(m), C.byref(st)))
        out = self._result(res, E, refine)
        if maps:
            out["maps"] = m
        return (out, locate_stats(st)) if stats else out

    def locate_device(self, picks, weights=None, min_picks=None, maps=False, refine=True, stats=False):
        import torch
        who = "Locator.locate_device"
        for name, a, dt in (("picks", picks, torch.float64), ("weights", weights, torch.float64), ("min_picks", min_picks, torch.int32)):
            if a is None:
                continue
            if not isinstance(a, torch.Tensor):
                raise TypeError(f"{who}: {name} must be a torch tensor")
            if a.dtype != dt:
                raise TypeError(f"{who}: {name} must be {dt}")
            if not a.is_contiguous():
                raise ValueError(f"{who}: {name} must be contiguous")
            if not a.is_cuda:                          # which GPU it is on, the library checks against the handle's
                raise ValueError(f"{who}: {name} must be a tensor on a GPU, not on the host")
        if picks.dim() != 2 or picks.shape[1] != self.P:
            raise ValueError(f"{who}: picks must be [E, {self.P}]")
        E = picks.shape[0]
        if weights is not None and weights.shape != picks.shape:
            raise ValueError(f"{who}: weights must have the shape of picks")
        if min_picks is not None and tuple(min_picks.shape) != (E,):
            raise ValueError(f"{who}: min_picks must be [E]")
        h = self._open()
        res = (_lib.LocateResult * E)()
        m = torch.empty((E, self.ny, self.nx), dtype=torch.float64, device=picks.device) if maps else None
        st = _lib.LocateStats()
        torch.cuda.synchronize(picks.device)           # the library works on the null stream
        check(lib().rtmi_locate_dev(h, E, picks.data_ptr(), None if weights is None else weights.data_ptr(),
                                    None if min_picks is None else min_picks.data_ptr(), res, None if m is None else m.data_ptr(),
                                    C.byref(st)))
        out = self._result(res, E, refine)
        if maps:
            out["maps"] = m
        return (out, locate_stats(st)) if stats else out

    def _edt_result(self, res, E, refine):
        a = np.frombuffer(res, dtype=np.dtype(_lib.EdtResult)).copy() if E else np.zeros(0, dtype=np.dtype(_lib.EdtResult))
        out = {"node": a["node"].copy(), "ix": a["ix"].copy(), "iy": a["iy"].copy(), "count": a["n"].copy(), "npairs": a["npairs"].copy(),
               "value": a["value"].copy(), "ref": a["ref"].copy(), "t0_node": a["t0"].copy(), "share_sum": a["share_sum"].copy(),
               "win_val": a["win_val"].reshape(E, 3, 3).copy(), "win_tau": a["win_tau"].reshape(E, 3, 3).copy()}
        if refine:
            out.update(x=a["x"].copy(), y=a["y"].copy(), t0=a["t0_refined"].copy(), dx=a["dx"].copy(), dy=a["dy"].copy(),
                       refined=a["refined"].copy())
        else:
            gx0, gdx, _, gy0, gdy, _ = self.grid
            none = out["node"] < 0
            out.update(x=np.where(none, np.nan, float(gx0) + out["ix"] * float(gdx)), y=np.where(none, np.nan, float(gy0) + out["iy"] * float(gdy)),
                       t0=out["t0_node"].copy(), dx=np.where(none, np.nan, 0.0), dy=np.where(none, np.nan, 0.0),
                       refined=np.zeros(E, dtype=np.int32))
        return out

    @staticmethod
    def _edt_params(sigma, chunks_per_group):
        ep = _lib.EdtParams()
        ep.sigma = float(sigma)
        ep.reserved[0] = int(chunks_per_group)
        return ep

    def locate_edt(self, picks, sigma, weights=None, min_picks=None, maps=False, refine=True, shares=False, stats=False,
                   _chunks_per_group=0):
        """Robust location by equal differential time (rtmi_locate_edt, include/rtmi.h): the node where the most
        station pairs agree on their traveltime difference within sigma, whatever the origin time.  One bad pick spoils only its
        own pairs, where `locate`'s least squares moves by cells.  picks, weights, min_picks as in `locate` (at least two picks
        must contribute); sigma is the pick error in seconds, or with weights (1 / sigma_r^2) a floor for the model's error added
        to every pick's variance (then it may be 0).  Returns a dict of arrays over the events:
          x, y, t0         the refined location and origin time where the refinement is accepted, else the node's own
          node, ix, iy     the best node (-1: no node has two and min_picks contributing picks); count, npairs, value in [0, 1]
          win_val, win_tau [E, 3, 3], dx, dy, refined, t0_node, ref, share_sum; with maps=True also maps [E, ny, nx]
          share, resid [E, P] with shares=True: each station's part of the best node's sum -- the station with a far smaller share
                           than the others holds the bad pick -- and its residual against t0_node; NaN where it does not contribute
        locate_edt_device takes torch tensors on the handle's device and returns maps, share and resid as tensors on it."""
        who = "Locator.locate_edt"
        t = np.ascontiguousarray(picks, dtype=np.float64)
        if t.ndim != 2 or t.shape[1] != self.P:
            raise ValueError(f"{who}: picks must be [E, {self.P}]")
        E = t.shape[0]
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        if w is not None and w.shape != t.shape:
            raise ValueError(f"{who}: weights must have the shape of picks")
        need = None
        if min_picks is not None:
            need = np.ascontiguousarray(np.broadcast_to(np.asarray(min_picks, dtype=np.int32), (E,)))
        ep = self._edt_params(sigma, _chunks_per_group)
        h = self._open()
        res = (_lib.EdtResult * E)()
        m = np.empty((E, self.ny, self.nx)) if maps else None
        sh = np.empty((E, self.P)) if shares else None
        rs = np.empty((E, self.P)) if shares else None
        st = _lib.LocateStats()
        check(lib().rtmi_locate_edt(h, C.byref(ep), E, dptr(t), dptr(w), None if need is None else need.ctypes.data_as(_lib._ip), res,
                                    dptr(sh), dptr(rs), dptr(m), C.byref(st)))
        out = self._edt_result(res, E, refine)
        if maps:
            out["maps"] = m
        if shares:
            out.update(share=sh, resid=rs)
        return (out, edt_stats(st)) if stats else out

    def locate_edt_device(self, picks, sigma, weights=None, min_picks=None, maps=False, refine=True, shares=False, stats=False,
                          _chunks_per_group=0):
        import torch
        who = "Locator.locate_edt_device"
        for name, a, dt in (("picks", picks, torch.float64), ("weights", weights, torch.float64), ("min_picks", min_picks, torch.int32)):
            if a is None:
                continue
            if not isinstance(a, torch.Tensor):
                raise TypeError(f"{who}: {name} must be a torch tensor")
            if a.dtype != dt:
                raise TypeError(f"{who}: {name} must be {dt}")
            if not a.is_contiguous():
                raise ValueError(f"{who}: {name} must be contiguous")
            if not a.is_cuda:                          # which GPU it is on, the library checks against the handle's
                raise ValueError(f"{who}: {name} must be a tensor on a GPU, not on the host")
        if picks is None or picks.dim() != 2 or picks.shape[1] != self.P:
            raise ValueError(f"{who}: picks must be [E, {self.P}]")
        E = picks.shape[0]
        if weights is not None and weights.shape != picks.shape:
            raise ValueError(f"{who}: weights must have the shape of picks")
        if min_picks is not None and tuple(min_picks.shape) != (E,):
            raise ValueError(f"{who}: min_picks must be [E]")
        ep = self._edt_params(sigma, _chunks_per_group)
        h = self._open()
        res = (_lib.EdtResult * E)()
        dev = picks.device
        m = torch.empty((E, self.ny, self.nx), dtype=torch.float64, device=dev) if maps else None
        sh = torch.empty((E, self.P), dtype=torch.float64, device=dev) if shares else None
        rs = torch.empty((E, self.P), dtype=torch.float64, device=dev) if shares else None
        st = _lib.LocateStats()
        p = lambda a: None if a is None else a.data_ptr()                                    # noqa: E731
        torch.cuda.synchronize(dev)                    # the library works on the null stream
        check(lib().rtmi_locate_edt_dev(h, C.byref(ep), E, p(picks), p(weights), p(min_picks), res, p(sh), p(rs), p(m), C.byref(st)))
        out = self._edt_result(res, E, refine)
        if maps:
            out["maps"] = m
        if shares:
            out.update(share=sh, resid=rs)
        return (out, edt_stats(st)) if stats else out

    def _pdf_params(self, who, method, sigma, power, levels, samples, group, tiles):
        if method not in ("l2", "edt"):
            raise ValueError(f"{who}: method must be 'l2' or 'edt'")
        levels = tuple(float(c) for c in levels)
        if len(levels) > 8:
            raise ValueError(f"{who}: at most 8 levels")
        pp = _lib.PdfParams()
        pp.sigma, pp.power, pp.nlevels, pp.S = float(sigma), int(power), len(levels), int(samples)
        for k, c in enumerate(levels):
            pp.levels[k] = c
        pp.reserved[0], pp.reserved[1] = int(group), int(tiles)
        return pp

    def _pdf_result(self, pdf, E, nlevels):
        a = np.frombuffer(pdf, dtype=np.dtype(_lib.PdfResult)).copy() if E else np.zeros(0, dtype=np.dtype(_lib.PdfResult))
        c = a["cov"].reshape(E, 3)
        cov = np.empty((E, 2, 2))
        cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 0], cov[:, 1, 1] = c[:, 0], c[:, 1], c[:, 1], c[:, 2]
        out = {"mean_x": a["mean_x"].copy(), "mean_y": a["mean_y"].copy(), "pdf_cov": cov, "ellipse": a["ellipse"].reshape(E, 3).copy(),
               "area": a["area"].copy(), "rim_fraction": a["rim_fraction"].copy(), "nz": a["nz"].copy(), "mass": a["mass"].copy()}
        for k in ("level_count", "level_area", "level_fraction", "level_rho"):
            out[k] = a[k].reshape(E, 8)[:, :nlevels].copy()
        return out

    def _sample_places(self, node, rng, jitter):
        """x, y of sampled nodes (NaN for -1), with a uniform offset within the cell where jitter"""
        gx0, gdx, _, gy0, gdy, _ = self.grid
        none = node < 0
        ix, iy = (node % self.nx).astype(np.float64), (node // self.nx).astype(np.float64)
        if jitter:
            ix = ix + rng.uniform(-0.5, 0.5, node.shape)
            iy = iy + rng.uniform(-0.5, 0.5, node.shape)
        return np.where(none, np.nan, float(gx0) + ix * float(gdx)), np.where(none, np.nan, float(gy0) + iy * float(gdy))

    def pdf(self, picks, sigma, method="l2", weights=None, min_picks=None, power=0, levels=(0.68, 0.95), marginals=False, samples=0,
            seed=0, jitter=True, u=None, stats=False, _events_per_group=0, _tiles_per_block=0, _chunks_per_group=0):
        """The location pdf of every event from the search's whole map, on the device (rtmi_locate_pdf, rtmi_locate_edt_pdf,
        include/rtmi.h): where `locate`'s cov is a quadratic through nine nodes, this sums over all of them, so a
        second lobe, a trade-off along a ray or a pdf cut off by the rim show.  method "l2": the density is
        exp(-sw (obj - obj*) / (2 sigma^2)); with weights in 1 / s^2 pass sigma = 1, without weights the picks' standard
        deviation.  method "edt": sigma is locate_edt's, the density is (value / value*)^power, power 0: the best node's number
        of readings.  Returns the search's own keys (bit-equal to locate / locate_edt) and
          mean_x, mean_y          the expectation
          pdf_cov [E, 2, 2]       the covariance about it; ellipse [E, 3]: semi-axes and the major one's angle from +x
          area                    the pdf's area in peak units; rim_fraction: the mass on the grid's rim; nz: the nodes with mass
          level_count, level_area, level_fraction, level_rho [E, len(levels)]: the highest-density region that holds each level
          mx [E, nx], my [E, ny]  with marginals=True
          sample_node [E, S], sample_x, sample_y with samples=S: drawn with numpy.random.default_rng(seed), with a uniform
                                  offset within the cell where jitter; u [E, S] in [0, 1) replaces the seeded uniforms
        An event with no candidate or no pdf has counts 0 and NaN.  pdf_device takes torch tensors on the handle's device and
        returns mx, my and sample_node as tensors on it (and no sample_x, sample_y)."""
        who = "Locator.pdf"
        pp = self._pdf_params(who, method, sigma, power, levels, samples, _events_per_group, _tiles_per_block)
        t = np.ascontiguousarray(picks, dtype=np.float64)
        if t.ndim != 2 or t.shape[1] != self.P:
            raise ValueError(f"{who}: picks must be [E, {self.P}]")
        E, S = t.shape[0], int(samples)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        if w is not None and w.shape != t.shape:
            raise ValueError(f"{who}: weights must have the shape of picks")
        need = None
        if min_picks is not None:
            need = np.ascontiguousarray(np.broadcast_to(np.asarray(min_picks, dtype=np.int32), (E,)))
        h = self._open()
        pdf = (_lib.PdfResult * E)()
        mx = np.empty((E, self.nx)) if marginals else None
        my = np.empty((E, self.ny)) if marginals else None
        rng = np.random.default_rng(seed)              # the uniforms first, then the offsets within the cell
        if S > 0:
            u = rng.random((E, S)) if u is None else np.ascontiguousarray(u, dtype=np.float64)
            if u.shape != (E, S):
                raise ValueError(f"{who}: u must be [E, samples]")
        else:
            u = None
        sm = np.empty((E, S), dtype=np.int32) if S > 0 else None
        st = _lib.LocateStats()
        ip = lambda a: None if a is None else a.ctypes.data_as(_lib._ip)                     # noqa: E731
        if method == "l2":
            res = (_lib.LocateResult * E)()
            check(lib().rtmi_locate_pdf(h, C.byref(pp), E, dptr(t), dptr(w), ip(need), res, pdf, dptr(mx), dptr(my), dptr(u), ip(sm),
                                        C.byref(st)))
            out = self._result(res, E, True)
        else:
            ep = self._edt_params(sigma, _chunks_per_group)
            res = (_lib.EdtResult * E)()
            check(lib().rtmi_locate_edt_pdf(h, C.byref(ep), C.byref(pp), E, dptr(t), dptr(w), ip(need), res, pdf, dptr(mx), dptr(my),
                                            dptr(u), ip(sm), C.byref(st)))
            out = self._edt_result(res, E, True)
        out.update(self._pdf_result(pdf, E, pp.nlevels))
        if marginals:
            out.update(mx=mx, my=my)
        if S > 0:
            x, y = self._sample_places(sm, rng, jitter)
            out.update(sample_node=sm, sample_x=x, sample_y=y, sample_u=u)
        return (out, pdf_stats(st)) if stats else out

    def pdf_device(self, picks, sigma, method="l2", weights=None, min_picks=None, power=0, levels=(0.68, 0.95), marginals=False,
                   samples=0, seed=0, u=None, stats=False, _events_per_group=0, _tiles_per_block=0, _chunks_per_group=0):
        """`pdf` on torch tensors of the handle's device; u [E, samples] (fp64, on the device) replaces the seeded draw"""
        import torch
        who = "Locator.pdf_device"
        for name, a, dt in (("picks", picks, torch.float64), ("weights", weights, torch.float64), ("min_picks", min_picks, torch.int32),
                            ("u", u, torch.float64)):
            if a is None:
                continue
            if not isinstance(a, torch.Tensor):
                raise TypeError(f"{who}: {name} must be a torch tensor")
            if a.dtype != dt:
                raise TypeError(f"{who}: {name} must be {dt}")
            if not a.is_contiguous():
                raise ValueError(f"{who}: {name} must be contiguous")
            if not a.is_cuda:                          # which GPU it is on, the library checks against the handle's
                raise ValueError(f"{who}: {name} must be a tensor on a GPU, not on the host")
        pp = self._pdf_params(who, method, sigma, power, levels, samples, _events_per_group, _tiles_per_block)
        if picks is None or picks.dim() != 2 or picks.shape[1] != self.P:
            raise ValueError(f"{who}: picks must be [E, {self.P}]")
        E, S = picks.shape[0], int(samples)
        if weights is not None and weights.shape != picks.shape:
            raise ValueError(f"{who}: weights must have the shape of picks")
        if min_picks is not None and tuple(min_picks.shape) != (E,):
            raise ValueError(f"{who}: min_picks must be [E]")
        if u is not None and tuple(u.shape) != (E, S):
            raise ValueError(f"{who}: u must be [E, samples]")
        h = self._open()
        dev = picks.device
        pdf = (_lib.PdfResult * E)()
        mx = torch.empty((E, self.nx), dtype=torch.float64, device=dev) if marginals else None
        my = torch.empty((E, self.ny), dtype=torch.float64, device=dev) if marginals else None
        if S > 0 and u is None:
            u = torch.from_numpy(np.random.default_rng(seed).random((E, S))).to(dev)
        sm = torch.empty((E, S), dtype=torch.int32, device=dev) if S > 0 else None
        st = _lib.LocateStats()
        p = lambda a: None if a is None else a.data_ptr()                                    # noqa: E731
        torch.cuda.synchronize(dev)                    # the library works on the null stream
        if method == "l2":
            res = (_lib.LocateResult * E)()
            check(lib().rtmi_locate_pdf_dev(h, C.byref(pp), E, p(picks), p(weights), p(min_picks), res, pdf, p(mx), p(my), p(u), p(sm),
                                            C.byref(st)))
            out = self._result(res, E, True)
        else:
            ep = self._edt_params(sigma, _chunks_per_group)
            res = (_lib.EdtResult * E)()
            check(lib().rtmi_locate_edt_pdf_dev(h, C.byref(ep), C.byref(pp), E, p(picks), p(weights), p(min_picks), res, pdf, p(mx), p(my),
                                                p(u), p(sm), C.byref(st)))
            out = self._edt_result(res, E, True)
        out.update(self._pdf_result(pdf, E, pp.nlevels))
        if marginals:
            out.update(mx=mx, my=my)
        if S > 0:
            out.update(sample_node=sm, sample_u=u)
        return (out, pdf_stats(st)) if stats else out

    def _stack_params(self, who, nt, dt, t0, scan, min_stations, threshold, min_sep, max_events):
        o0, od, M = scan
        sp = _lib.StackParams()
        sp.nt, sp.M, sp.ct0, sp.cdt, sp.o0, sp.od = int(nt), int(M), float(t0), float(dt), float(o0), float(od)
        sp.need = 0 if min_stations is None else int(min_stations)
        sp.threshold, sp.min_sep, sp.max_events = float(threshold), int(min_sep), int(max_events)
        return sp

    def _stack_events(self, ev, K, sp, refine):
        a = np.frombuffer(ev, dtype=np.dtype(_lib.StackEvent))[:K].copy() if K else np.zeros(0, dtype=np.dtype(_lib.StackEvent))
        out = {"m": a["m"].copy(), "node": a["node"].copy(), "ix": a["ix"].copy(), "iy": a["iy"].copy(), "count": a["n"].copy(),
               "value": a["value"].copy(), "t0_node": a["t0"].copy(), "win": a["win"].reshape(K, 3, 3, 3).copy()}
        if refine:
            out.update(x=a["x"].copy(), y=a["y"].copy(), t0=a["t0_refined"].copy(), dx=a["dx"].copy(), dy=a["dy"].copy(),
                       dm=a["dm"].copy(), refined=a["refined"].copy())
        else:
            gx0, gdx, _, gy0, gdy, _ = self.grid
            out.update(x=float(gx0) + out["ix"] * float(gdx), y=float(gy0) + out["iy"] * float(gdy), t0=out["t0_node"].copy(),
                       dx=np.zeros(K), dy=np.zeros(K), dm=np.zeros(K), refined=np.zeros(K, dtype=np.int32))
        return out

    def stack(self, traces, dt, t0=0.0, scan=(0.0, 1.0, 1), weights=None, min_stations=None, threshold=np.inf, min_sep=0, max_events=0,
              maps=False, volume=False, refine=True, stats=False):
        """Pick-free detection and location (rtmi_locate_stack, include/rtmi.h): traces [P, nt], one characteristic
        function per station (an envelope, STA/LTA, kurtosis: computing it is the caller's job; NaN marks a gap), sample i at time
        t0 + i dt, are stacked along every node's moveout for the origin times o0 + m od, m < M, of scan = (o0, od, M).
        weights [P]: a station with a weight that is 0, negative or not finite is left out.  min_stations: the fewest stations
        that must contribute to a node (default: every valid one).  Returns a dict:
          peak, peak_node [M]   the detection series: the greatest stack of each origin time and the node that attains it
                                (-inf and -1 where no node has enough stations)
          m, node, ix, iy, count, value, t0_node, win [K, 3, 3, 3]   the events: the at most max_events greatest samples of peak
                                that reach threshold, at least min_sep + 1 scan indices apart, in the order they are taken
          x, y, t0, dx, dy, dm, refined   their refined location (bit 0 of refined) and origin time (bit 1); with refine=False
                                the node's own
          best, best_m [ny, nx] with maps=True: each node's greatest stack over the scan and its scan index;
          volume [M, ny, nx] with volume=True: the stack itself.
        stack_device takes traces and weights as torch tensors on the handle's device and returns peak, peak_node, best, best_m
        and volume as tensors on it.  With stats=True the calls return (result, stats)."""
        who = "Locator.stack"
        c = np.ascontiguousarray(traces, dtype=np.float64)
        if c.ndim != 2 or c.shape[0] != self.P:
            raise ValueError(f"{who}: traces must be [{self.P}, nt]")
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        if w is not None and w.shape != (self.P,):
            raise ValueError(f"{who}: weights must be [{self.P}]")
        sp = self._stack_params(who, c.shape[1], dt, t0, scan, min_stations, threshold, min_sep, max_events)
        h = self._open()
        M = max(int(sp.M), 0)
        peak, peak_node = np.empty(M), np.empty(M, dtype=np.int32)
        best = np.empty((self.ny, self.nx)) if maps else None
        best_m = np.empty((self.ny, self.nx), dtype=np.int32) if maps else None
        vol = np.empty((M, self.ny, self.nx)) if volume else None
        ev = (_lib.StackEvent * max(int(sp.max_events), 1))()
        nev, st = C.c_int64(0), _lib.StackStats()
        ip = lambda a: None if a is None else a.ctypes.data_as(_lib._ip)                     # noqa: E731
        check(lib().rtmi_locate_stack(h, C.byref(sp), dptr(c), dptr(w), dptr(peak), ip(peak_node), dptr(best), ip(best_m), dptr(vol),
                                      ev, C.byref(nev), C.byref(st)))
        out = self._stack_events(ev, int(nev.value), sp, refine)
        out.update(peak=peak, peak_node=peak_node)
        if maps:
            out.update(best=best, best_m=best_m)
        if volume:
            out["volume"] = vol
        return (out, stack_stats(st)) if stats else out

    def stack_device(self, traces, dt, t0=0.0, scan=(0.0, 1.0, 1), weights=None, min_stations=None, threshold=np.inf, min_sep=0,
                     max_events=0, maps=False, volume=False, refine=True, stats=False):
        import torch
        who = "Locator.stack_device"
        for name, a in (("traces", traces), ("weights", weights)):
            if a is None:
                continue
            if not isinstance(a, torch.Tensor):
                raise TypeError(f"{who}: {name} must be a torch tensor")
            if a.dtype != torch.float64:
                raise TypeError(f"{who}: {name} must be {torch.float64}")
            if not a.is_contiguous():
                raise ValueError(f"{who}: {name} must be contiguous")
            if not a.is_cuda:                          # which GPU it is on, the library checks against the handle's
                raise ValueError(f"{who}: {name} must be a tensor on a GPU, not on the host")
        if traces is None or traces.dim() != 2 or traces.shape[0] != self.P:
            raise ValueError(f"{who}: traces must be [{self.P}, nt]")
        if weights is not None and tuple(weights.shape) != (self.P,):
            raise ValueError(f"{who}: weights must be [{self.P}]")
        sp = self._stack_params(who, traces.shape[1], dt, t0, scan, min_stations, threshold, min_sep, max_events)
        h = self._open()
        M, dev = max(int(sp.M), 0), traces.device
        peak = torch.empty(M, dtype=torch.float64, device=dev)
        peak_node = torch.empty(M, dtype=torch.int32, device=dev)
        best = torch.empty((self.ny, self.nx), dtype=torch.float64, device=dev) if maps else None
        best_m = torch.empty((self.ny, self.nx), dtype=torch.int32, device=dev) if maps else None
        vol = torch.empty((M, self.ny, self.nx), dtype=torch.float64, device=dev) if volume else None
        ev = (_lib.StackEvent * max(int(sp.max_events), 1))()
        nev, st = C.c_int64(0), _lib.StackStats()
        p = lambda a: None if a is None else a.data_ptr()                                    # noqa: E731
        torch.cuda.synchronize(dev)                    # the library works on the null stream
        check(lib().rtmi_locate_stack_dev(h, C.byref(sp), p(traces), p(weights), p(peak), p(peak_node), p(best), p(best_m), p(vol),
                                          ev, C.byref(nev), C.byref(st)))
        out = self._stack_events(ev, int(nev.value), sp, refine)
        out.update(peak=peak, peak_node=peak_node)
        if maps:
            out.update(best=best, best_m=best_m)
        if volume:
            out["volume"] = vol
        return (out, stack_stats(st)) if stats else out

    def close(self):
        if self._h:
            lib().rtmi_locator_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def debug_fix_norm(x):
    """rtmi_debug_fix_norm: the device's order-independent norm of a host vector -> (norm, e)"""
    xx = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    nrm = C.c_double()
    e = C.c_int32()
    check(lib().rtmi_debug_fix_norm(dptr(xx), xx.size, C.byref(nrm), C.byref(e)))
    return nrm.value, int(e.value)


def first_arrivals(selected_func, field, sources, line, receivers_u, **kw):
    """The [S, J] table of first-arrival traveltimes (NaN where no ray converged): two_point's smallest T."""
    r = two_point(selected_func, field, sources, line, receivers_u, **kw)
    return np.where(r["count"] > 0, r["T"][..., 0], np.nan)


def device_sincos(x):
    """The library's libm-identical fp64 sin and cos (rtmi_debug_sincos), evaluated on the device -> (sin, cos)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    s = np.empty_like(x); c = np.empty_like(x)
    check(lib().rtmi_debug_sincos(x.size, dptr(x), dptr(s), dptr(c)))
    return s, c


def device_arctan2(y, x):
    """The library's restatement of numpy's float64 arctan2 (rtmi_debug_arctan2: rt::ex::atan2_), evaluated on the device."""
    y, x = np.broadcast_arrays(np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64))
    y = np.ascontiguousarray(y); x = np.ascontiguousarray(x)
    out = np.empty_like(x)
    check(lib().rtmi_debug_arctan2(x.size, dptr(y), dptr(x), dptr(out)))
    return out


def device_exp(x):
    """The field build's restatement of numpy's float64 array exp (rtmi_debug_exp: np_exp of k_sample), evaluated on the device."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    check(lib().rtmi_debug_exp(x.size, dptr(x), dptr(out)))
    return out


def device_rcp14_table():
    """The VRCP14PD table device_arctan2 reads, as decoded on the current device (rtmi_debug_rcp14_table) -> uint16 [65536]."""
    out = np.empty(65536, dtype=np.uint16)
    check(lib().rtmi_debug_rcp14_table(out.ctypes.data_as(C.POINTER(C.c_uint16))))
    return out


_ACC = ("x", "y", "theta", "dist_sim", "dist_real", "T")


def launch_is_coherent(x0, y0, theta, group=64):
    """True when consecutive rays already travel together (sorted fans do): within most groups of `group`
    consecutive rays the launch points coincide to a fraction of a cell and the angles span no more than a few
    times the batch's mean angular spacing per group.  Used by sort_rays="auto"."""
    th = np.asarray(theta, dtype=np.float64)
    R = len(th)
    if R < 2 * group:
        return True
    n = (R // group) * group
    g = th[:n].reshape(-1, group)
    with np.errstate(invalid="ignore"):
        spread = np.nanmax(g, axis=1) - np.nanmin(g, axis=1)
        total = np.nanmax(th) - np.nanmin(th)
    fair = 8.0 * total * group / R + 1e-12
    xs = np.asarray(x0, dtype=np.float64)[:n].reshape(-1, group)
    ys = np.asarray(y0, dtype=np.float64)[:n].reshape(-1, group)
    same_origin = (np.ptp(xs, axis=1) < DELTA) & (np.ptp(ys, axis=1) < DELTA)
    return bool(np.mean((spread <= fair) & same_origin) > 0.75)


def max_rows(user_choice, step, divisor):
    """max_size of trazar (:796-799)."""
    c = constants(user_choice)
    return N * divisor if c[10] else int(np.ceil(c[4] / step) + 1)


def snell_angles(s_ray, d_ray, theta_v):
    """Interface exit angles (:896-919) per ray, degrees: (angsim, angreal) -- the simulated outward angle over
    the second-to-last 5 % of the trajectory and the Snell / reflection angle it should have."""
    R = s_ray.shape[2]
    angsim, angreal = np.zeros(R), np.zeros(R)
    for k in range(R):
        i = int(d_ray[2, k])
        th = theta_v[k]
        if th < np.pi / 4:
            angreal[k] = 90 - 180 * th / np.pi
        elif th == np.pi / 4:
            angreal[k] = 0
        else:
            angreal[k] = 180 * np.arcsin(np.sqrt(2) * np.sin(np.pi / 2 - th)) / np.pi
        a, b = int(9.5 * i / 10), int(9 * i / 10)
        distx = s_ray[a, 0, k] - s_ray[b, 0, k]
        disty = s_ray[a, 1, k] - s_ray[b, 1, k]
        with np.errstate(divide="ignore", invalid="ignore"):
            angsim[k] = 180 * np.arctan(np.abs(distx / disty)) / np.pi
    return angsim, angreal


def snell_errors(s_ray, d_ray, theta_v):
    """Host restatement of the exit-angle error (:918); the library evaluates it on the device (rtmi_metric)."""
    angsim, angreal = snell_angles(s_ray, d_ray, theta_v)
    return np.abs(angsim - angreal)


def _format_num(num):
    """The reference's column formatter (:929-943)."""
    if num < 0:
        return "{: >10.8f}".format(num) if abs(num) < 10 else "{: >10.7f}".format(num)
    return "{: >10.9f}".format(num) if num < 10 else "{: >10.8f}".format(num)


def closure_error(s_ray):
    """Fisheye closure error in % of 2*pi (:956, :1393)."""
    return 100 * np.linalg.norm(np.array([1, 0]) - s_ray[-1, 0:2, 0]) / (2 * np.pi)


def moment_cv(s_ray, ray_count=None):
    """Mean coefficient of variation (%) of p_x over rays 1..R-2 (:1354-1360, :1398-1402)."""
    ray_count = s_ray.shape[2] if ray_count is None else ray_count
    cvs = np.zeros(ray_count - 2)
    for i in range(1, ray_count - 1):
        masked = np.ma.masked_equal(s_ray[:, 2, i], 0).compressed()
        cvs[i - 1] = 100 * np.std(masked) / np.mean(masked)
    return np.mean(cvs)


def trazar_plan(user_choice, step, divisor, thetas=None, starts=None, box=None, gamma=None, max_size=None, record="full"):
    """What trazar's preamble settles before any ray moves (RT_bench.py:793-804): the launch conditions, the box, gamma,
    max_size and the record stride, from the preset of `user_choice` and the keyword overrides.  Needs no device."""
    g, ray_count, theta_v, pos_x, s, limx_i, limx_s, limy_i, limy_s, op_if, op_fish, _, _ = constants(user_choice)
    if thetas is not None:
        theta_v = np.asarray(thetas, dtype=np.float64)
        ray_count = len(theta_v)
    if starts is not None:
        st = np.asarray(starts, dtype=np.float64)
        x0, y0 = (st[0], st[1]) if st.ndim == 1 else (st[:, 0], st[:, 1])
    elif op_fish:
        x0, y0 = float(pos_x[0]), float(pos_x[1])            # :810
    else:
        px = np.asarray(pos_x, dtype=np.float64)
        x0 = px[:ray_count] if len(px) >= ray_count else np.full(ray_count, px[0])
        y0 = -2.0                                            # :812
    if max_size is None:
        max_size = N * divisor if op_fish else int(np.ceil(s / step) + 1)   # :796-799
    stride = 0 if record is None else (1 if record == "full" else int(record))
    return dict(ray_count=int(ray_count), theta_v=np.asarray(theta_v, dtype=np.float64)[:ray_count], x0=x0, y0=y0,
                box=(limx_i, limx_s, limy_i, limy_s) if box is None else box, gamma=g if gamma is None else gamma,
                max_size=int(max_size), stride=stride, rec_rows=(int(max_size) + stride - 1) // stride if stride else 0,
                op_interface=bool(op_if), op_fisheye=bool(op_fish))


def trazar(selected_func, z, grd, show, step, divisor, user_choice, *, thetas=None, starts=None, box=None,
           gamma=None, max_size=None, record="full", return_batch=False, launch_mode="auto", reference_order=False,
           read_rows=True):
    """RT_bench.py:766-948 on the GPU.  Positional arguments and the returned
    (s_ray[max_size,6,R], d_ray[3,R], compute_times[R], errors[R]) are the reference's.

    Keyword extensions for synthetic batches: thetas / starts ((R,2) or (2,)) / box / gamma / max_size replace
    the preset of `user_choice`; record = "full" (reference layout), an int stride, or None (s_ray is None).
    compute_times holds the device propagation time split evenly over rays, so np.sum(compute_times) is the
    quantity the reference's benchmark reads (:1526).  launch_mode: "auto" (rtmi_params' default: the library picks the
    schedule), "plain", "refill", "sliced" or the rtmi_launch_mode integer -- same bits in all of them.  reference_order=True:
    op1/2/6/8 too step in the reference's own operation order (rtmi_params.reference_order; op7 always does): they then return
    the oracle's bits (the reference's, within 1 ulp where numpy's scalar pow(x, 2) is not x*x), at about a third of the speed.
    read_rows=False (with return_batch=True): leave the recorded rows on the device (s_ray is returned as None; take them
    from Batch.device_tensors() / Batch.rows()).
    """
    pl = trazar_plan(user_choice, step, divisor, thetas, starts, box, gamma, max_size, record)
    fld = _field_of(z, grd)
    ray_count, theta_v, stride = pl["ray_count"], pl["theta_v"], pl["stride"]
    b = Batch(fld, selected_func, step, pl["max_size"], pl["box"], pl["gamma"], theta_v, pl["x0"], pl["y0"], record_stride=stride,
              sort_rays="auto", keep_n_ray=False,          # n_ray is internal to the reference's trazar (:803), never returned
              launch_mode=launch_mode, reference_order=reference_order)
    t1 = time.perf_counter()
    b.run()
    b.sync()
    t2 = time.perf_counter()
    st_ = b.stats()
    d_ray = b.d_ray()
    s_ray = b.rows() if stride and read_rows else None
    compute_times = np.full(ray_count, (st_["kernel_ms"] * 1e-3 if st_["kernel_ms"] > 0 else t2 - t1) / ray_count)
    errors = np.zeros(ray_count)
    if pl["op_interface"] and stride == 1:
        errors = b.metric("snell")          # (:896-919) evaluated on the device
        if show and s_ray is not None:   # the reference's per-ray table (:921-945)
            print_exit_table(s_ray, d_ray, errors, theta_v)
    if return_batch:
        return s_ray, d_ray, compute_times, errors, b
    b.close()
    return s_ray, d_ray, compute_times, errors


def print_exit_table(s_ray, d_ray, errors, theta_v):
    """The reference's per-ray table of the interface scenario (RT_bench.py:921-945)."""
    angsim, angreal = snell_angles(s_ray, d_ray, theta_v)
    f = _format_num
    for k in range(s_ray.shape[2]):
        i = int(d_ray[2, k])
        print(f"Coords: [ {f(s_ray[i, 0, k])} , {f(s_ray[i, 1, k])} ] | SimAng: {f(angsim[k])} | "
              f"SnellAng: {f(angreal[k])} | Err: {f(errors[k])} | InitAng: {f(theta_v[k] * 180 / np.pi)}")


def search_delta(option, z, grd, step, divisor, user_choice):
    """RT_bench.py:950-958."""
    c = constants(user_choice)
    rays, _, _, errors = trazar(option, z, grd, False, step, divisor, user_choice)
    if c[9]:
        return np.mean(errors), np.max(errors)
    if c[10]:
        return closure_error(rays)
    return rays[:, 2, :]


# --------------------------------------------------------------------------- calibration + benchmark harness
# (the reference's other consumer of trazar, restated over the GPU path)
def calibrated_delta_s(user_choice, method_choice):
    """The hard-coded calibrated DELTA_S table (RT_bench.py:1412-1455).  method_choice is the menu entry "1".."9"
    (isotropic) or "1"/"2" (anisotropic).  Returns (DELTA_S, DELTA_S_DIVISOR_FISHEYE or None)."""
    c = constants(user_choice)
    m = str(method_choice)
    if c[9] or c[11]:
        div = {"1": 38.64, "2": 38.37, "3": 2.34, "4": 2.53, "5": 2.53, "6": 2.55, "7": 30.05, "8": 2.74, "9": 2.74}[m]
        return SIGMA / div, None
    if c[10]:
        div = {"1": 4587, "2": 4556, "3": 278, "4": 300, "5": 300, "6": 303, "7": 3567, "8": 325, "9": 325}[m]
        return 2 * np.pi / div, div
    return SIGMA / (2.53 if m == "1" else 2.74), None


def delta_s_candidates(user_choice):
    """(divisors, delta_s_options) of the DELTA_S search (RT_bench.py:1302-1312)."""
    c = constants(user_choice)
    if c[9]:
        divisors = np.arange(DELTA_S_DIVISOR_UPPER_LIMIT, DELTA_S_DIVISOR_LOWER_LIMIT - DELTA_STEP, -DELTA_STEP)
        return divisors, SIGMA / divisors
    if c[10]:
        divisors = np.arange(DELTA_S_DIVISOR_FISHEYE_UPPER_LIMIT, DELTA_S_DIVISOR_FISHEYE_LOWER_LIMIT - DELTA_STEP_FISHEYE,
                             -DELTA_STEP_FISHEYE)
        return divisors, 2 * np.pi / divisors
    divisors = np.arange(DELTA_S_DIVISOR_VERT_UPPER_LIMIT, DELTA_S_DIVISOR_VERT_LOWER_LIMIT - 2 * DELTA_STEP, -DELTA_STEP)
    return divisors, SIGMA / divisors


def search_delta_sweep(option, z, grd, delta_s_options, divisors, user_choice, batched=True):
    """What executor.map(search_delta, ...) returns (RT_bench.py:1317-1318): one entry per DELTA_S candidate --
    (mean, max) exit-angle error for interface, closure % for fisheye, mean p_x CV (%) for the vert scenarios
    (the reference returns the p_x history there and reduces it at :1354-1360; the reduction runs on the device).

    batched=True runs the whole sweep as ONE candidate x ray batch (every ray carries its candidate's DELTA_S and
    max_size, rtmi_batch_set_per_ray) followed by one device metric; batched=False runs one small batch per
    candidate.  Both give the same bits per ray."""
    c = constants(user_choice)
    g, ray_count, theta_v, pos_x, s, xi, xs, yi, ys, op_if, op_fish, _, _ = c
    fld = _field_of(z, grd)
    steps = [float(v) for v in delta_s_options]
    sizes = [int(N * d) if op_fish else int(np.ceil(s / st) + 1) for st, d in zip(steps, np.asarray(divisors) + 1)]
    th = np.asarray(theta_v, dtype=np.float64)[:ray_count]
    x0, y0 = (float(pos_x[0]), float(pos_x[1])) if op_fish else (np.asarray(pos_x, float)[:ray_count], -2.0)
    stride = 0 if op_fish else 1
    kind = "snell" if op_if else ("closure" if op_fish else "px_cv")

    def reduce_(m):
        if op_if:
            return (np.mean(m), np.max(m))
        return m[0] if op_fish else np.mean(m[1:ray_count - 1])

    if not batched:
        out = []
        for st, ms in zip(steps, sizes):
            b = Batch(fld, option, st, ms, (xi, xs, yi, ys), g, th, x0, y0, record_stride=stride)
            b.run()
            out.append(reduce_(b.metric(kind)))
            b.close()
        return out
    nc = len(steps)
    b = Batch(fld, option, steps[0], max(sizes), (xi, xs, yi, ys), g, np.tile(th, nc),
              np.tile(np.broadcast_to(x0, (ray_count,)), nc), np.tile(np.broadcast_to(y0, (ray_count,)), nc),
              record_stride=stride)
    b.set_per_ray(np.repeat(steps, ray_count), np.repeat(sizes, ray_count))
    b.run()
    m = b.metric(kind).reshape(nc, ray_count)
    b.close()
    return [reduce_(m[i]) for i in range(nc)]


def find_divisor(results, divisors, user_choice, max_deviation=None):
    """The three find_index rules of the DELTA_S search (RT_bench.py:1320-1385) -> chosen divisor or None."""
    c = constants(user_choice)
    if c[9]:
        md = MAX_DEVIATION if max_deviation is None else max_deviation
        errors = [r[0] for r in results]; max_errors = [r[1] for r in results]
        if not any(e > md for e in errors) or not any(e < md for e in errors):
            return None
        for i in reversed(range(len(errors))):
            if errors[i] < md and max_errors[i] < 0.8:
                if all(e < md for e in errors[:i]) and all(e < 0.8 for e in max_errors[:i]):
                    return round(divisors[i], 2)
        return None
    if c[10]:
        md = 5 if max_deviation is None else max_deviation
        errors = list(results)
        if not any(e > md for e in errors) or not any(e < md for e in errors):
            return None
        for i in range(len(errors)):
            if errors[i] > md:
                return round(divisors[i - 1])
        return None
    md = 0.05 if max_deviation is None else max_deviation
    errors = list(results)
    if not any(e > md for e in errors) or not any(e < md for e in errors):
        return None
    for i in range(len(errors)):
        if i > 1 and errors[i] > md and all(e < md for e in errors[:i - 1]):
            return round(divisors[i - 1], 2)
    return None


def remove_outliers_iqr(data):
    """RT_bench.py:123-138."""
    data = np.asarray(data)
    q1, q3 = np.percentile(data, 25), np.percentile(data, 75)
    iqr = q3 - q1
    return data[(data >= q1 - 1.5 * iqr) & (data <= q3 + 1.5 * iqr)]


def benchmark(option, z, grd, step, divisor, user_choice, trial=100, replicas=3, max_rounds=20, **kw):
    """The reference's benchmark statistic (RT_bench.py:1516-1541) over device propagation times: rounds of
    trial*replicas runs, IQR filter, median of the last 30 %, repeat until two successive medians differ by
    < 0.5 %; returns the mean of the last two ("Completion time per scenario", seconds)."""
    _, _, _, _, b = trazar(option, z, grd, False, step, divisor, user_choice, record=None, return_batch=True, **kw)
    benchmarks = []
    try:
        for _ in range(max_rounds):
            arr = np.zeros(trial * replicas)
            for j in range(trial * replicas):
                b.reset()
                b.run()
                arr[j] = b.stats()["kernel_ms"] * 1e-3
            cleaned = remove_outliers_iqr(arr)
            benchmarks.append(np.median(cleaned[int(-0.3 * len(cleaned)):]))
            if len(benchmarks) >= 2:
                if 100 * abs(benchmarks[-1] - benchmarks[-2]) / max(benchmarks[-1], benchmarks[-2]) < 0.5:
                    break
    finally:
        b.close()
    return float(np.mean(benchmarks[-2:]))
