"""ctypes binding of oracle/librt_oracle.so (the CPU restatement, rt_oracle.c).

TEST INFRASTRUCTURE ONLY: import this from tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg -- never from raytracing_amd/.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# two builds of rt_oracle.c: "default" squares with x*x (what the device reproduces); "pow" squares like the reference's numpy
# scalars do, with libm pow(x, 2.0) (see SQ() in rt_oracle.c) -- the reference-faithful build the fixtures are ALSO checked with
_SOS = {"default": os.path.join(_HERE, "librt_oracle.so"), "pow": os.path.join(_HERE, "librt_oracle_pow.so")}
_SO = _SOS["default"]

SCENARIOS = {"interface": 1, "fisheye": 2, "vert_heterogeneous": 3, "anisotropy": 4}

_dp = C.POINTER(C.c_double)


def build(force=False, variant="default"):
    src = os.path.join(_HERE, "rt_oracle.c")
    so = _SOS[variant]
    if force or not os.path.exists(so) or (os.path.exists(src) and os.path.getmtime(so) < os.path.getmtime(src)):
        subprocess.check_call(["make", "-C", _HERE, "-s", os.path.basename(so)])
    return so


class _Params(C.Structure):
    _fields_ = [("method", C.c_int), ("gamma", C.c_double), ("gamma_step", C.c_double), ("step", C.c_double),
                ("max_size", C.c_int), ("box", C.c_double * 4), ("record_stride", C.c_int),
                ("rec_rows", C.c_long), ("nthreads", C.c_int)]


_libs = {}
_variant = "default"


def variant(name):
    """Context manager: calls inside use the named build ("default" | "pow").  Fields remember the build they came from."""
    import contextlib

    @contextlib.contextmanager
    def cm():
        global _variant
        old, _variant = _variant, name
        try:
            yield
        finally:
            _variant = old
    return cm()


def lib(which=None):
    which = which or _variant
    if which not in _libs:
        L = C.CDLL(build(variant=which))
        L.rto_field_build.restype = C.c_void_p
        L.rto_field_build.argtypes = [C.c_int] + [C.c_double] * 5
        L.rto_field_from_samples.restype = C.c_void_p
        L.rto_field_from_samples.argtypes = [_dp, C.c_int, _dp, C.c_int, _dp, C.c_double]
        L.rto_field_free.argtypes = [C.c_void_p]
        L.rto_field_dims.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.rto_field_get.argtypes = [C.c_void_p] + [_dp] * 5
        L.rto_n_gradient_many.argtypes = [C.c_void_p, C.c_int] + [_dp] * 5
        L.rto_single_step.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, _dp, _dp, _dp]
        L.rto_trazar.restype = C.c_long
        L.rto_trazar.argtypes = [C.c_void_p, C.POINTER(_Params), C.c_int] + [_dp] * 7
        L.rto_trazar_from_state.restype = C.c_long
        L.rto_trazar_from_state.argtypes = [C.c_void_p, C.POINTER(_Params), C.c_int, _dp, _dp, C.POINTER(C.c_int)] + [_dp] * 4
        L.rto_max_threads.restype = C.c_int
        L.rto_set_field_solver.argtypes = [C.c_int]
        L.rto_np_exp_many.argtypes = [_dp, _dp, C.c_long]
        L.rto_np_arctan2_many.argtypes = [_dp, _dp, _dp, C.c_long]
        _libs[which] = L
    return _libs[which]


def set_field_solver(lu):
    """0 (default): FITPACK's Givens QR, the reference's bits; 1: the banded LU rounds 1-2 used (1.3e-15 away)."""
    lib().rto_set_field_solver(int(lu))


def np_exp(x):
    """The oracle's restatement of numpy's float64 array exp (SVML __svml_exp8_ha), for tools/check_np_exp.py."""
    x = _f64(x); y = np.empty_like(x)
    lib().rto_np_exp_many(_p(x), _p(y), x.size)
    return y


def _p(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def np_arctan2(y, x):
    """The oracle's restatement of numpy's float64 arctan2 (SVML __svml_atan28_ha), for tools/check_np_atan2.py."""
    y = _f64(y); x = _f64(x); o = np.empty_like(x)
    lib().rto_np_arctan2_many(_p(y), _p(x), _p(o), x.size)
    return o


class Field:
    """genZ + interpolacion (RT_bench.py:412-464) restated on the CPU."""

    def __init__(self, scenario, limits, delta):
        sc = SCENARIOS[scenario] if isinstance(scenario, str) else int(scenario)
        self.L = lib()
        self.h = self.L.rto_field_build(sc, *[float(v) for v in limits], float(delta))
        qx, qy = C.c_int(), C.c_int()
        self.L.rto_field_dims(self.h, C.byref(qx), C.byref(qy))
        self.qx, self.qy = qx.value, qy.value

    @classmethod
    def from_samples(cls, x, y, Z, delta):
        """interpolacion(x, y, Z, X, Y) (RT_bench.py:435) for caller-provided samples."""
        x = _f64(x); y = _f64(y); Z = _f64(Z)
        self = cls.__new__(cls)
        self.L = lib()
        self.h = self.L.rto_field_from_samples(_p(x), len(x), _p(y), len(y), _p(Z), float(delta))
        self.qx, self.qy = len(x), len(y)
        return self

    def arrays(self):
        x = np.empty(self.qx); y = np.empty(self.qy)
        Z = np.empty((self.qy, self.qx)); cdy = np.empty_like(Z); cdx = np.empty_like(Z)
        self.L.rto_field_get(self.h, _p(x), _p(y), _p(Z), _p(cdy), _p(cdx))
        return x, y, Z, cdy, cdx

    def n_gradient(self, x, y):
        x = _f64(np.atleast_1d(x)); y = _f64(np.atleast_1d(y))
        n = np.empty_like(x); gx = np.empty_like(x); gy = np.empty_like(x)
        self.L.rto_n_gradient_many(self.h, len(x), _p(x), _p(y), _p(n), _p(gx), _p(gy))
        return n, gx, gy

    def __del__(self):
        if getattr(self, "h", None) and getattr(self, "L", None) is not None:
            self.L.rto_field_free(self.h)
            self.h = None


def single_step(field, method, gamma, step, st, hist=None):
    st = _f64(st); out = np.empty((st.shape[0], 6))
    hist = _f64(hist) if hist is not None else None
    for q in range(st.shape[0]):
        field.L.rto_single_step(field.h, method, float(gamma), float(step), _p(st[q]),
                              _p(hist[q]) if hist is not None else None, _p(out[q]))
    return out


def _params(method, gamma, step, max_size, box, record_stride, nthreads, gamma_step):
    p = _Params()
    p.method = int(method); p.gamma = float(gamma)
    p.gamma_step = float(gamma if gamma_step is None else gamma_step)
    p.step = float(step); p.max_size = int(max_size)
    for i in range(4):
        p.box[i] = float(box[i])
    p.record_stride = int(record_stride); p.nthreads = int(nthreads)
    return p


def _outputs(p, R, max_size, record_stride, rec_rows, want_n_ray):
    s_ray = n_ray = None
    if record_stride:
        rows = int(rec_rows) if rec_rows is not None else (int(max_size) + record_stride - 1) // record_stride
        p.rec_rows = rows
        s_ray = np.zeros((rows, 6, R))
        n_ray = np.zeros((rows, R)) if want_n_ray else None
    return s_ray, n_ray, np.zeros((3, R)), np.zeros((9, R))


def trazar(field, method, gamma, step, max_size, box, x0, y0, theta0, record_stride=1, rec_rows=None,
           nthreads=1, gamma_step=None, want_n_ray=False):
    """RT_bench.py:766-948.  Returns dict(s_ray [rows,6,R] or None, n_ray, d_ray [3,R], final [9,R], steps)."""
    th = _f64(theta0); R = len(th)
    x0 = _f64(np.broadcast_to(x0, (R,))); y0 = _f64(np.broadcast_to(y0, (R,)))
    p = _params(method, gamma, step, max_size, box, record_stride, nthreads, gamma_step)
    s_ray, n_ray, d_ray, final = _outputs(p, R, max_size, record_stride, rec_rows, want_n_ray)
    steps = field.L.rto_trazar(field.h, C.byref(p), R, _p(x0), _p(y0), _p(th), _p(s_ray), _p(n_ray), _p(d_ray),
                             _p(final))
    return dict(s_ray=s_ray, n_ray=n_ray, d_ray=d_ray, final=final, steps=int(steps))


def trazar_from_state(field, method, gamma, step, max_size, box, state9, hist4=None, istep=0, record_stride=1, rec_rows=None,
                      nthreads=1, gamma_step=None, want_n_ray=False):
    """trazar's loop (:866-879) continued from a given state, as rtmi_batch_set_state asks of the device.
    state9 [9,R] = x, y, theta, n, dn/dx, dn/dy, dist_sim, dist_real, T; hist4 [4,R] (op7) = the two positions before,
    oldest first (x, y, x, y); istep [R] (or one int) = the row each state is at.  Rows after istep only are written (the
    others stay 0).  Returns what trazar returns; d_ray holds dist_real, dist_sim, last row (NOT state9's order)."""
    st = _f64(state9); R = st.shape[1]
    assert st.shape == (9, R)
    h = None
    if hist4 is not None:
        h = _f64(hist4)
        assert h.shape == (4, R)
    elif int(method) == 7:
        raise ValueError("op7 needs hist4 (the two positions before each state)")
    ist = np.ascontiguousarray(np.broadcast_to(np.asarray(istep, dtype=np.int32), (R,)))
    p = _params(method, gamma, step, max_size, box, record_stride, nthreads, gamma_step)
    s_ray, n_ray, d_ray, final = _outputs(p, R, max_size, record_stride, rec_rows, want_n_ray)
    steps = field.L.rto_trazar_from_state(field.h, C.byref(p), R, _p(st), _p(h), ist.ctypes.data_as(C.POINTER(C.c_int)),
                                          _p(s_ray), _p(n_ray), _p(d_ray), _p(final))
    return dict(s_ray=s_ray, n_ray=n_ray, d_ray=d_ray, final=final, steps=int(steps))


def max_threads():
    return lib().rto_max_threads()
