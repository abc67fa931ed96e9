"""ctypes binding of librtmi.so (include/rtmi.h).  No fallback: if the HIP library is missing or a
call fails this raises -- the product path never computes on the CPU."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RTMI_LIB_PATH: load another build of the same ABI (A/B timing of kernel variants in one session)
LIB_PATH = os.environ.get("RTMI_LIB_PATH") or os.path.join(_HERE, "librtmi.so")

ABI_VERSION = 7
AUTO_SAMPLES = 3        # RTMI_AUTO_SAMPLES (include/rtmi.h)
# rtmi_launch_mode (include/rtmi.h)
LAUNCH_AUTO, LAUNCH_REFILL, LAUNCH_SLICED, LAUNCH_PLAIN = 0, 1, 2, 3
LAUNCH_MODES = {"auto": LAUNCH_AUTO, "refill": LAUNCH_REFILL, "sliced": LAUNCH_SLICED, "plain": LAUNCH_PLAIN, "lane": LAUNCH_PLAIN}
LAUNCH_NAMES = {LAUNCH_AUTO: "auto", LAUNCH_REFILL: "refill", LAUNCH_SLICED: "sliced", LAUNCH_PLAIN: "plain"}

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class RtmiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"librtmi error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    _fields_ = [("method", C.c_int32), ("dtype", C.c_int32), ("gamma", C.c_double), ("gamma_step", C.c_double),
                ("step", C.c_double), ("max_size", C.c_int32), ("record_stride", C.c_int32), ("rec_rows", C.c_int64),
                ("box", C.c_double * 4), ("launch_mode", C.c_int32), ("block_size", C.c_int32),
                ("refill_min", C.c_int32), ("exact_basis", C.c_int32),
                ("field_path", C.c_int32), ("sort_rays", C.c_int32),
                ("ext_s_ray", C.c_void_p), ("ext_n_ray", C.c_void_p), ("lazy_clear", C.c_int32), ("no_n_ray", C.c_int32), ("slice_steps", C.c_int32),
                ("reference_order", C.c_int32), ("no_retrace", C.c_int32)]


class DeviceView(C.Structure):
    _fields_ = [("s_ray", C.c_void_p), ("n_ray", C.c_void_p), ("x", C.c_void_p), ("y", C.c_void_p),
                ("theta", C.c_void_p), ("n", C.c_void_p), ("gx", C.c_void_p), ("gy", C.c_void_p),
                ("dist_sim", C.c_void_p), ("dist_real", C.c_void_p), ("T", C.c_void_p), ("istep", C.c_void_p),
                ("perm", C.c_void_p),
                ("R", C.c_int64), ("rec_rows", C.c_int64), ("dtype", C.c_int32), ("record_stride", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("ray_steps", C.c_uint64), ("live_rays", C.c_uint64), ("kernel_ms", C.c_double),
                ("launches", C.c_uint32), ("vgprs", C.c_uint32), ("sgprs", C.c_uint32), ("lds_bytes", C.c_uint32),
                ("launch_mode_used", C.c_uint32), ("kernel_ms_total", C.c_double), ("launches_total", C.c_uint64),
                ("auto_fallbacks", C.c_uint32), ("auto_kept", C.c_uint32),
                ("auto_ms", (C.c_double * AUTO_SAMPLES) * 2), ("auto_n", C.c_uint32 * 2),
                ("retraced", C.c_uint32), ("retrace_overflow", C.c_uint32), ("retraced_total", C.c_uint64),
                ("dispatch_first", C.c_uint32), ("reserved_", C.c_uint32)]


class ShardStats(C.Structure):
    _fields_ = [("ndev", C.c_int32), ("transport", C.c_int32), ("R", C.c_int64), ("ray_steps", C.c_uint64), ("live_rays", C.c_uint64),
                ("run_seconds", C.c_double), ("kernel_ms_max", C.c_double), ("auto_fallbacks", C.c_uint32), ("reserved_", C.c_uint32)]


class TwoPointParams(C.Structure):
    _fields_ = [("max_arrivals", C.c_int32), ("max_crossings", C.c_int32), ("max_iter", C.c_int32), ("reserved0", C.c_int32),
                ("tol", C.c_double), ("mem_budget", C.c_int64), ("reserved", C.c_int64 * 4)]


class TwoPointStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("groups", C.c_int32), ("rec_rows", C.c_int64), ("overflow", C.c_uint64),
                ("fan_ms", C.c_double), ("bracket_ms", C.c_double), ("refine_ms", C.c_double), ("reserved", C.c_double * 4)]


class GridParams(C.Structure):
    _fields_ = [("gx0", C.c_double), ("gdx", C.c_double), ("nx", C.c_int64), ("gy0", C.c_double), ("gdy", C.c_double),
                ("ny", C.c_int64), ("max_gap", C.c_double), ("max_dtheta", C.c_double), ("amplitude", C.c_int32),
                ("reserved0", C.c_int32), ("reserved", C.c_int64 * 4)]


class GridStats(C.Structure):
    _fields_ = [("cells", C.c_int64), ("skipped_cells", C.c_int64), ("triangles", C.c_int64), ("folded", C.c_int64),
                ("atomics", C.c_uint64 * 3), ("pass_ms", C.c_double * 3), ("max_gap", C.c_double), ("max_dtheta", C.c_double),
                ("reserved", C.c_double * 4)]


class ArrivalParams(C.Structure):
    _fields_ = [("karr", C.c_int32), ("order", C.c_int32), ("reserved", C.c_int64 * 4)]


class ArrivalStats(C.Structure):
    _fields_ = GridStats._fields_ + [("candidates", C.c_int64), ("scan_ms", C.c_double)]


class SensitivityStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("atomics", C.c_int64), ("scale_exp", C.c_int32), ("reserved0", C.c_int32),
                ("reserved", C.c_int64 * 4)]


class BeamParams(C.Structure):
    _fields_ = [("gx0", C.c_double), ("gdx", C.c_double), ("nx", C.c_int64), ("gy0", C.c_double), ("gdy", C.c_double),
                ("ny", C.c_int64), ("eps", C.c_double), ("cutoff", C.c_double), ("max_width", C.c_double),
                ("edge_taper", C.c_double), ("reserved", C.c_int64 * 4)]


class BeamStats(C.Structure):
    _fields_ = [("segments", C.c_int64), ("tile_entries", C.c_int64), ("pairs_tested", C.c_int64), ("pairs_inside", C.c_int64),
                ("capped", C.c_int64), ("prep_ms", C.c_double), ("bin_ms", C.c_double), ("gather_ms", C.c_double),
                ("cutoff", C.c_double), ("max_width", C.c_double), ("reserved", C.c_double * 4)]


class KirchhoffParams(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("P", C.c_int64), ("N", C.c_int64), ("nt", C.c_int64),
                ("t0", C.c_double), ("dt", C.c_double), ("nbin", C.c_int32), ("reserved0", C.c_int32), ("dopen", C.c_double),
                ("reserved", C.c_int64 * 4)]


class KirchhoffMultiParams(C.Structure):
    """rtmi_kirchhoff_multi_params: KirchhoffParams with karr where that has reserved0"""
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("P", C.c_int64), ("N", C.c_int64), ("nt", C.c_int64),
                ("t0", C.c_double), ("dt", C.c_double), ("nbin", C.c_int32), ("karr", C.c_int32), ("dopen", C.c_double),
                ("reserved", C.c_int64 * 4)]


KIRCHHOFF_MAX_ARRIVALS = 4
KIRCHHOFF_MAX_LEVELS = 8


class KirchhoffAAParams(C.Structure):
    """rtmi_kirchhoff_aa_params: KirchhoffMultiParams, then the levels and the trace spacings of the anti-aliased pair"""
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("P", C.c_int64), ("N", C.c_int64), ("nt", C.c_int64),
                ("t0", C.c_double), ("dt", C.c_double), ("nbin", C.c_int32), ("karr", C.c_int32), ("dopen", C.c_double),
                ("nlev", C.c_int32), ("reserved0", C.c_int32), ("hw", C.c_int32 * KIRCHHOFF_MAX_LEVELS),
                ("asrc", C.c_double), ("arec", C.c_double), ("amid", C.c_double), ("reserved", C.c_int64 * 4)]


class KirchhoffStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("upload_ms", C.c_double), ("pairs", C.c_int64), ("contributing", C.c_int64),
                ("scale_exp", C.c_int32), ("reserved0", C.c_int32), ("reserved", C.c_int64 * 4)]


class LsqrParams(C.Structure):
    _fields_ = [("iter_lim", C.c_int32), ("reserved0", C.c_int32), ("damp", C.c_double), ("atol", C.c_double), ("btol", C.c_double),
                ("reserved", C.c_int64 * 4)]


class LsqrStats(C.Structure):
    _fields_ = [("istop", C.c_int32), ("itn", C.c_int32), ("r1norm", C.c_double), ("r2norm", C.c_double), ("anorm", C.c_double),
                ("arnorm", C.c_double), ("total_ms", C.c_double), ("operator_ms", C.c_double), ("vector_ms", C.c_double),
                ("bytes_device", C.c_int64), ("reserved", C.c_int64 * 4)]


class LsqrOptions(C.Structure):
    """rtmi_lsqr_options: host fp64 vectors, any of them NULL"""
    _fields_ = [("row_weight", _dp), ("col_scale", _dp), ("x0", _dp), ("reserved", C.c_int64 * 5)]


class TomoStats(C.Structure):
    _fields_ = [("rows", C.c_int64), ("segments", C.c_int64), ("padded_segments", C.c_int64), ("bytes_device", C.c_int64),
                ("atomics", C.c_int64), ("compile_ms", C.c_double), ("kernel_ms", C.c_double), ("vmax", C.c_double),
                ("qx", C.c_int32), ("qy", C.c_int32), ("scale_exp", C.c_int32), ("reserved0", C.c_int32), ("reserved", C.c_int64 * 4)]


class TomoReg(C.Structure):
    """rtmi_tomo_reg: the first- and second-difference weights of rtmi_tomo_lsqr_basis, {lx, ly} and {mx2, my2}"""
    _fields_ = [("d1", C.c_double * 2), ("d2", C.c_double * 2), ("reserved", C.c_int64 * 4)]


class LocatorParams(C.Structure):
    """rtmi_locator_params: the grid of the tables and their number"""
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("P", C.c_int64), ("gx0", C.c_double), ("gdx", C.c_double),
                ("gy0", C.c_double), ("gdy", C.c_double), ("reserved", C.c_int64 * 4)]


class LocateResult(C.Structure):
    """rtmi_locate_result: one event's best node, its 3 x 3 windows and the refined location"""
    _fields_ = [("node", C.c_int32), ("ix", C.c_int32), ("iy", C.c_int32), ("n", C.c_int32), ("sw", C.c_double), ("obj", C.c_double),
                ("ref", C.c_double), ("t0", C.c_double), ("win_obj", C.c_double * 9), ("win_tau", C.c_double * 9), ("x", C.c_double),
                ("y", C.c_double), ("t0_refined", C.c_double), ("dx", C.c_double), ("dy", C.c_double), ("cov", C.c_double * 3),
                ("refined", C.c_int32), ("reserved0", C.c_int32), ("reserved", C.c_int64 * 2)]


class LocateStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("upload_ms", C.c_double), ("triples", C.c_int64), ("contributing", C.c_int64),
                ("reserved", C.c_int64 * 4)]


class EdtParams(C.Structure):
    """rtmi_edt_params: the pick error (or, with weights, the model-error floor) of rtmi_locate_edt"""
    _fields_ = [("sigma", C.c_double), ("reserved", C.c_int64 * 4)]


class EdtResult(C.Structure):
    """rtmi_edt_result: one event's best node by equal differential time, its 3 x 3 windows and the refined location"""
    _fields_ = [("node", C.c_int64), ("ix", C.c_int64), ("iy", C.c_int64), ("n", C.c_int64), ("npairs", C.c_int64),
                ("value", C.c_double), ("ref", C.c_double), ("t0", C.c_double), ("share_sum", C.c_double),
                ("win_val", C.c_double * 9), ("win_tau", C.c_double * 9), ("x", C.c_double), ("y", C.c_double),
                ("t0_refined", C.c_double), ("dx", C.c_double), ("dy", C.c_double), ("refined", C.c_int32), ("reserved0", C.c_int32),
                ("reserved", C.c_int64 * 2)]


class PdfParams(C.Structure):
    """rtmi_pdf_params: the density's scale (least squares) or power (EDT), the confidence levels and the samples per event of
    rtmi_locate_pdf and rtmi_locate_edt_pdf"""
    _fields_ = [("sigma", C.c_double), ("power", C.c_int32), ("nlevels", C.c_int32), ("levels", C.c_double * 8), ("S", C.c_int64),
                ("reserved", C.c_int64 * 4)]


class PdfResult(C.Structure):
    """rtmi_pdf_result: one event's expectation, covariance, ellipse, area, rim fraction and confidence regions"""
    _fields_ = [("mean_x", C.c_double), ("mean_y", C.c_double), ("cov", C.c_double * 3), ("ellipse", C.c_double * 3),
                ("area", C.c_double), ("rim_fraction", C.c_double), ("nz", C.c_int64), ("mass", C.c_int64),
                ("level_count", C.c_int64 * 8), ("level_area", C.c_double * 8), ("level_fraction", C.c_double * 8),
                ("level_rho", C.c_double * 8), ("reserved", C.c_int64 * 4)]


class EikonalParams(C.Structure):
    """rtmi_eikonal_params: the grid as in GridParams, the source ball's radius in cells, the cap on the rounds and the fill's scheme"""
    _fields_ = [("gx0", C.c_double), ("gdx", C.c_double), ("nx", C.c_int64), ("gy0", C.c_double), ("gdy", C.c_double),
                ("ny", C.c_int64), ("ball", C.c_double), ("max_rounds", C.c_int32), ("scheme", C.c_int32),
                ("reserved", C.c_int64 * 4)]


class EikonalStats(C.Structure):
    _fields_ = [("free_nodes", C.c_int64), ("filled", C.c_int64), ("unreached", C.c_int64), ("changes", C.c_int64),
                ("rounds_max", C.c_int32), ("path", C.c_int32), ("kernel_ms", C.c_double), ("reserved", C.c_int64 * 4)]


class EikonalTomoStats(C.Structure):
    """rtmi_eikonal_tomo_stats: the shape and the live rows of an eikonal tomography handle, and the times of its last product"""
    _fields_ = [("rows", C.c_int64), ("live_rows", C.c_int64), ("S", C.c_int64), ("R", C.c_int64), ("nx", C.c_int64),
                ("ny", C.c_int64), ("touched", C.c_int64), ("bytes_device", C.c_int64), ("self_filled", C.c_int32),
                ("path", C.c_int32), ("rounds_max", C.c_int32), ("reserved0", C.c_int32), ("sweep_ms", C.c_double),
                ("kernel_ms", C.c_double), ("reduce_ms", C.c_double), ("reserved", C.c_int64 * 3)]


EIKONAL_LDS, EIKONAL_GLOBAL = 1, 2      # rtmi_eikonal_stats.path
EIKONAL_PATHS = {EIKONAL_LDS: "lds", EIKONAL_GLOBAL: "global"}
EIKONAL_PLAIN, EIKONAL_FACTORED, EIKONAL_FACTORED_LIN = 0, 1, 3  # rtmi_eikonal_params.scheme
EIKONAL_SCHEMES = {"plain": EIKONAL_PLAIN, "factored": EIKONAL_FACTORED}
EIKONAL_LINEARISE = ("plain", "factored")  # the linearisation of the tangent and adjoint entries; "factored" is EIKONAL_FACTORED_LIN


class StackParams(C.Structure):
    """rtmi_stack_params: the trace axis, the origin-time scan and the event selection of rtmi_locate_stack"""
    _fields_ = [("nt", C.c_int64), ("M", C.c_int64), ("ct0", C.c_double), ("cdt", C.c_double), ("o0", C.c_double), ("od", C.c_double),
                ("need", C.c_int64), ("threshold", C.c_double), ("min_sep", C.c_int64), ("max_events", C.c_int64),
                ("reserved", C.c_int64 * 4)]


class StackEvent(C.Structure):
    """rtmi_stack_event: one event of the stack, its 3 x 3 x 3 window and the refined location and origin time"""
    _fields_ = [("m", C.c_int32), ("node", C.c_int32), ("ix", C.c_int32), ("iy", C.c_int32), ("n", C.c_int32), ("reserved0", C.c_int32),
                ("value", C.c_double), ("t0", C.c_double), ("win", C.c_double * 27), ("x", C.c_double), ("y", C.c_double),
                ("t0_refined", C.c_double), ("dx", C.c_double), ("dy", C.c_double), ("dm", C.c_double), ("refined", C.c_int32),
                ("reserved1", C.c_int32), ("reserved", C.c_int64 * 2)]


class StackStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("upload_ms", C.c_double), ("triples", C.c_int64), ("contributing", C.c_int64),
                ("truncated", C.c_int32), ("reserved0", C.c_int32), ("reserved", C.c_int64 * 4)]


LOCATE_MAX_TABLES = 512  # RTMI_LOCATE_MAX_TABLES: the most tables (stations) of a locator
TOMO_SKIP = -2          # RTMI_TOMO_SKIP: rtmi_tomo_append's `which` for a ray without a row
LSQR_RANGE = 8          # RTMI_LSQR_RANGE: rtmi_kirchhoff_lsqr's own istop
LSQR_OP_PLAIN, LSQR_OP_FULL, LSQR_OP_FILTERED = 0, 1, 2     # RTMI_LSQR_OP_: rtmi_kirchhoff_lsqr_weighted's operator
LSQR_MULTI_MAX = 64     # RTMI_LSQR_MULTI_MAX: the most columns of one rtmi_tomo_*_multi call
LSQR_MULTI_ROW_WEIGHT = 1   # RTMI_LSQR_MULTI_ROW_WEIGHT: rtmi_tomo_lsqr_multi's row_weight is [nrhs][rows]
HILBERT_MAX_NT = 16384  # the longest trace rtmi_kirchhoff_hilbert takes: one copy of it in LDS
FILTER_MAX_NT = 16384   # the longest trace and ...
FILTER_MAX_TAPS = 2048  # ... the most taps rtmi_kirchhoff_set_filter takes: the trace and the filter's zeros in LDS

# rtmi_arrival_grid's orders and largest karr
ARRIVAL_BY_TIME, ARRIVAL_BY_AMPLITUDE, MAX_ARRIVALS = 0, 1, 16
ARRIVAL_ORDERS = {"time": ARRIVAL_BY_TIME, "amplitude": ARRIVAL_BY_AMPLITUDE}
# rtmi_arrival_status
ARRIVAL_EMPTY, ARRIVAL_CONVERGED, ARRIVAL_STALLED, ARRIVAL_TRUNCATED = -1, 1, 2, 3

SHARD_AUTO, SHARD_RCCL, SHARD_COPY = 0, 1, 2
# every symbol include/rtmi.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "rtmi_abi_version": (C.c_int, []),
    "rtmi_last_error": (C.c_char_p, []),
    "rtmi_set_device": (C.c_int, [C.c_int]),
    "rtmi_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "rtmi_field_build": (C.c_int, [C.c_int] + [C.c_double] * 5 + [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "rtmi_field_from_samples": (C.c_int, [_dp, C.c_int, _dp, C.c_int, _dp, C.c_double, C.c_int, C.c_void_p,
                                          C.POINTER(C.c_void_p)]),
    "rtmi_field_dims": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rtmi_field_read": (C.c_int, [C.c_void_p] + [_dp] * 5),
    "rtmi_field_eval": (C.c_int, [C.c_void_p, C.c_int64] + [_dp] * 5),
    "rtmi_field_destroy": (None, [C.c_void_p]),
    "rtmi_batch_create": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_int64, _dp, _dp, _dp, C.c_void_p,
                                    C.POINTER(C.c_void_p)]),
    "rtmi_batch_set_state": (C.c_int, [C.c_void_p, _dp, _dp, _ip]),
    "rtmi_batch_get_state": (C.c_int, [C.c_void_p, _dp, _dp, _ip, C.c_void_p]),
    "rtmi_batch_restore_state": (C.c_int, [C.c_void_p, _dp, _dp, _ip, C.c_void_p]),
    "rtmi_batch_set_per_ray": (C.c_int, [C.c_void_p, _dp, _ip]),
    "rtmi_batch_reset": (C.c_int, [C.c_void_p]),
    "rtmi_step": (C.c_int, [C.c_void_p, C.c_int32]),
    "rtmi_step_repeat": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "rtmi_run": (C.c_int, [C.c_void_p]),
    "rtmi_sync": (C.c_int, [C.c_void_p]),
    "rtmi_read_d_ray": (C.c_int, [C.c_void_p, _dp]),
    "rtmi_read_final": (C.c_int, [C.c_void_p, _dp]),
    "rtmi_read_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _dp, _dp]),
    "rtmi_metric": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "rtmi_isochrones": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp]),
    "rtmi_wavefronts": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int32, C.POINTER(C.c_int64), _dp, _dp]),
    "rtmi_crossings": (C.c_int, [C.c_void_p, _dp, C.c_int32, _ip, _dp]),
    "rtmi_two_point": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_int32, _dp, _dp, C.c_int32, _dp, _dp, C.c_int32, _dp,
                                 C.POINTER(TwoPointParams), _ip, _ip, _dp, C.POINTER(TwoPointStats)]),
    "rtmi_paraxial": (C.c_int, [C.c_void_p, _dp, C.c_int32, _ip, _dp, _dp]),
    "rtmi_field_eval_dgrad": (C.c_int, [C.c_void_p, C.c_int64] + [_dp] * 6),
    "rtmi_first_arrival_grid": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(GridParams), _ip, _dp, C.POINTER(GridStats)]),
    "rtmi_arrival_grid": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(GridParams), C.POINTER(ArrivalParams), _ip, _dp,
                                    C.POINTER(ArrivalStats)]),
    "rtmi_traveltime_perturb": (C.c_int, [C.c_void_p, _dp, C.c_int32, _dp, _ip, _dp, _dp, C.POINTER(SensitivityStats)]),
    "rtmi_traveltime_backproject": (C.c_int, [C.c_void_p, _dp, C.c_int32, _dp, _dp, _dp, C.POINTER(SensitivityStats)]),
    "rtmi_gaussian_beams": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(BeamParams), C.c_int32, _dp, _dp, C.POINTER(BeamStats)]),
    "rtmi_kirchhoff_create": (C.c_int, [C.POINTER(KirchhoffParams), _dp, _dp, _dp, _ip, _ip, _dp, C.POINTER(C.c_void_p)]),
    "rtmi_kirchhoff_migrate": (C.c_int, [C.c_void_p, _dp, _dp, C.POINTER(KirchhoffStats)]),
    "rtmi_kirchhoff_model": (C.c_int, [C.c_void_p, _dp, _dp, C.POINTER(KirchhoffStats)]),
    "rtmi_kirchhoff_destroy": (None, [C.c_void_p]),
    "rtmi_kirchhoff_create_multi": (C.c_int, [C.POINTER(KirchhoffMultiParams), _dp, _dp, _dp, _dp, _ip, _ip, _dp,
                                              C.POINTER(C.c_void_p)]),
    "rtmi_kirchhoff_migrate2": (C.c_int, [C.c_void_p, _dp, _dp, _dp, C.POINTER(KirchhoffStats)]),
    "rtmi_kirchhoff_model2": (C.c_int, [C.c_void_p, _dp, _dp, _dp, C.POINTER(KirchhoffStats)]),
    "rtmi_kirchhoff_create_aa": (C.c_int, [C.POINTER(KirchhoffAAParams), _dp, _dp, _dp, _dp, _dp, _ip, _ip, _dp,
                                           C.POINTER(C.c_void_p)]),
    "rtmi_kirchhoff_aa_filter": (C.c_int, [C.c_void_p, _dp, _dp]),
    "rtmi_kirchhoff_migrate_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(KirchhoffStats)]),
    "rtmi_kirchhoff_model_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(KirchhoffStats)]),
    "rtmi_kirchhoff_lsqr": (C.c_int, [C.c_void_p, C.POINTER(LsqrParams), _dp, _dp, _dp, C.POINTER(LsqrStats)]),
    "rtmi_hilbert_taps": (C.c_int, [C.c_int64, _dp]),
    "rtmi_kirchhoff_hilbert": (C.c_int, [C.c_void_p, _dp, _dp]),
    "rtmi_kirchhoff_hilbert_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rtmi_kirchhoff_lsqr_full": (C.c_int, [C.c_void_p, C.POINTER(LsqrParams), _dp, _dp, _dp, C.POINTER(LsqrStats)]),
    "rtmi_half_derivative_taps": (C.c_int, [C.c_int64, C.c_double, _dp]),
    "rtmi_kirchhoff_set_filter": (C.c_int, [C.c_void_p, _dp, C.c_int64, C.c_int64]),
    "rtmi_kirchhoff_filter": (C.c_int, [C.c_void_p, _dp, C.c_int32, _dp]),
    "rtmi_kirchhoff_filter_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rtmi_kirchhoff_lsqr_filtered": (C.c_int, [C.c_void_p, C.POINTER(LsqrParams), _dp, _dp, _dp, C.POINTER(LsqrStats)]),
    "rtmi_tomo_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "rtmi_tomo_append": (C.c_int, [C.c_void_p, C.c_void_p, _dp, C.c_int32, _ip, _ip, C.POINTER(C.c_int64)]),
    "rtmi_tomo_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), _ip, _dp]),
    "rtmi_tomo_info": (C.c_int, [C.c_void_p, C.POINTER(TomoStats)]),
    "rtmi_tomo_apply": (C.c_int, [C.c_void_p, _dp, _dp, C.POINTER(TomoStats)]),
    "rtmi_tomo_apply_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TomoStats)]),
    "rtmi_tomo_transpose": (C.c_int, [C.c_void_p, _dp, _dp, C.POINTER(TomoStats)]),
    "rtmi_tomo_transpose_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TomoStats)]),
    "rtmi_tomo_lsqr": (C.c_int, [C.c_void_p, C.POINTER(LsqrParams), _dp, _dp, _dp, _dp, C.POINTER(LsqrStats)]),
    "rtmi_tomo_destroy": (None, [C.c_void_p]),
    "rtmi_kirchhoff_lsqr_weighted": (C.c_int, [C.c_void_p, C.POINTER(LsqrParams), C.POINTER(LsqrOptions), C.c_int32, _dp, _dp, _dp,
                                               C.POINTER(LsqrStats)]),
    "rtmi_tomo_lsqr_weighted": (C.c_int, [C.c_void_p, C.POINTER(LsqrParams), C.POINTER(LsqrOptions), _dp, _dp, _dp, _dp,
                                          C.POINTER(LsqrStats)]),
    "rtmi_kirchhoff_illumination": (C.c_int, [C.c_void_p, _dp, C.POINTER(KirchhoffStats)]),
    "rtmi_kirchhoff_illumination_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(KirchhoffStats)]),
    "rtmi_bspline_axis": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _ip, _dp]),
    "rtmi_tomo_basis_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _ip, _dp, C.c_int32, C.c_int32, _ip, _dp,
                                         C.POINTER(C.c_void_p)]),
    "rtmi_tomo_basis_prolong": (C.c_int, [C.c_void_p, _dp, _dp]),
    "rtmi_tomo_basis_restrict": (C.c_int, [C.c_void_p, _dp, _dp]),
    "rtmi_tomo_basis_prolong_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtmi_tomo_basis_restrict_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtmi_tomo_basis_destroy": (None, [C.c_void_p]),
    "rtmi_tomo_lsqr_basis": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(LsqrParams), C.POINTER(LsqrOptions), C.POINTER(TomoReg), _dp,
                                       _dp, _dp, _dp, C.POINTER(LsqrStats)]),
    "rtmi_tomo_apply_multi": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp, C.POINTER(TomoStats)]),
    "rtmi_tomo_apply_multi_dev": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(TomoStats)]),
    "rtmi_tomo_transpose_multi": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp, C.POINTER(TomoStats)]),
    "rtmi_tomo_transpose_multi_dev": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(TomoStats)]),
    "rtmi_tomo_lsqr_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(LsqrParams), C.POINTER(LsqrOptions), C.POINTER(TomoReg), C.c_int32,
                                       C.c_int32, _dp, _dp, _dp, _dp, C.POINTER(LsqrStats)]),
    "rtmi_locator_create": (C.c_int, [C.POINTER(LocatorParams), _dp, C.POINTER(C.c_void_p)]),
    "rtmi_locator_destroy": (None, [C.c_void_p]),
    "rtmi_locate": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp, _ip, C.POINTER(LocateResult), _dp, C.POINTER(LocateStats)]),
    "rtmi_locate_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(LocateResult), C.c_void_p,
                                  C.POINTER(LocateStats)]),
    "rtmi_locate_edt": (C.c_int, [C.c_void_p, C.POINTER(EdtParams), C.c_int64, _dp, _dp, _ip, C.POINTER(EdtResult), _dp, _dp, _dp,
                                  C.POINTER(LocateStats)]),
    "rtmi_locate_edt_dev": (C.c_int, [C.c_void_p, C.POINTER(EdtParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(EdtResult), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(LocateStats)]),
    "rtmi_edt_exp": (C.c_int, [_dp, _dp, C.c_int64]),
    "rtmi_locate_pdf": (C.c_int, [C.c_void_p, C.POINTER(PdfParams), C.c_int64, _dp, _dp, _ip, C.POINTER(LocateResult),
                                  C.POINTER(PdfResult), _dp, _dp, _dp, _ip, C.POINTER(LocateStats)]),
    "rtmi_locate_pdf_dev": (C.c_int, [C.c_void_p, C.POINTER(PdfParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(LocateResult), C.POINTER(PdfResult), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(LocateStats)]),
    "rtmi_locate_edt_pdf": (C.c_int, [C.c_void_p, C.POINTER(EdtParams), C.POINTER(PdfParams), C.c_int64, _dp, _dp, _ip,
                                      C.POINTER(EdtResult), C.POINTER(PdfResult), _dp, _dp, _dp, _ip, C.POINTER(LocateStats)]),
    "rtmi_locate_edt_pdf_dev": (C.c_int, [C.c_void_p, C.POINTER(EdtParams), C.POINTER(PdfParams), C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.POINTER(EdtResult), C.POINTER(PdfResult), C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.POINTER(LocateStats)]),
    "rtmi_eikonal_fill": (C.c_int, [C.POINTER(EikonalParams), _dp, C.c_int64, _dp, _dp, _dp, _ip, C.POINTER(C.c_uint8),
                                    C.POINTER(EikonalStats)]),
    "rtmi_eikonal_fill_dev": (C.c_int, [C.POINTER(EikonalParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, _ip,
                                        C.c_void_p, C.POINTER(EikonalStats)]),
    "rtmi_eikonal_tangent": (C.c_int, [C.POINTER(EikonalParams), _dp, C.c_int64, _dp, _dp, _dp, C.POINTER(C.c_uint8), _dp, _dp, _dp,
                                       _dp, _ip, C.POINTER(EikonalStats)]),
    "rtmi_eikonal_tangent_dev": (C.c_int, [C.POINTER(EikonalParams), C.c_void_p, C.c_int64] + [C.c_void_p] * 8 +
                                 [_ip, C.POINTER(EikonalStats)]),
    "rtmi_eikonal_adjoint": (C.c_int, [C.POINTER(EikonalParams), _dp, C.c_int64, _dp, _dp, _dp, C.POINTER(C.c_uint8), _dp, _dp, _dp,
                                       _dp, _ip, C.POINTER(EikonalStats)]),
    "rtmi_eikonal_adjoint_dev": (C.c_int, [C.POINTER(EikonalParams), C.c_void_p, C.c_int64] + [C.c_void_p] * 8 +
                                 [_ip, C.POINTER(EikonalStats)]),
    "rtmi_eikonal_tangent_multi": (C.c_int, [C.POINTER(EikonalParams), _dp, C.c_int64, _dp, _dp, _dp, C.POINTER(C.c_uint8), C.c_int32,
                                             _dp, _dp, _dp, _dp, _ip, C.POINTER(EikonalStats)]),
    "rtmi_eikonal_tangent_multi_dev": (C.c_int, [C.POINTER(EikonalParams), C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int32] +
                                       [C.c_void_p] * 4 + [_ip, C.POINTER(EikonalStats)]),
    "rtmi_eikonal_adjoint_multi": (C.c_int, [C.POINTER(EikonalParams), _dp, C.c_int64, _dp, _dp, _dp, C.POINTER(C.c_uint8), C.c_int32,
                                             _dp, _dp, _dp, _dp, _ip, C.POINTER(EikonalStats)]),
    "rtmi_eikonal_adjoint_multi_dev": (C.c_int, [C.POINTER(EikonalParams), C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int32] +
                                       [C.c_void_p] * 4 + [_ip, C.POINTER(EikonalStats)]),
    "rtmi_eikonal_attributes": (C.c_int, [C.POINTER(EikonalParams), _dp, C.c_int64, _dp, _dp, _dp, C.POINTER(C.c_uint8), _dp, _dp, _dp,
                                          _dp, _ip, C.POINTER(EikonalStats)]),
    "rtmi_eikonal_attributes_dev": (C.c_int, [C.POINTER(EikonalParams), C.c_void_p, C.c_int64] + [C.c_void_p] * 8 +
                                    [_ip, C.POINTER(EikonalStats)]),
    "rtmi_eikonal_tomo_create": (C.c_int, [C.POINTER(EikonalParams), _dp, C.c_int64, _dp, _dp, _dp, C.POINTER(C.c_uint8), C.c_int64, _dp,
                                           C.POINTER(C.c_void_p)]),
    "rtmi_eikonal_tomo_destroy": (None, [C.c_void_p]),
    "rtmi_eikonal_tomo_info": (C.c_int, [C.c_void_p, C.POINTER(EikonalTomoStats), C.POINTER(C.c_int64)]),
    "rtmi_eikonal_tomo_table": (C.c_int, [C.c_void_p, _dp, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "rtmi_eikonal_tomo_apply": (C.c_int, [C.c_void_p, _dp, _dp, C.POINTER(EikonalTomoStats)]),
    "rtmi_eikonal_tomo_apply_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EikonalTomoStats)]),
    "rtmi_eikonal_tomo_transpose": (C.c_int, [C.c_void_p, _dp, _dp, C.POINTER(EikonalTomoStats)]),
    "rtmi_eikonal_tomo_transpose_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EikonalTomoStats)]),
    "rtmi_eikonal_tomo_residual": (C.c_int, [C.c_void_p, _dp, _dp]),
    "rtmi_eikonal_tomo_residual_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtmi_eikonal_tomo_relinearise": (C.c_int, [C.c_void_p, _dp, _dp]),
    "rtmi_eikonal_tomo_relinearise_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtmi_eikonal_tomo_lsqr": (C.c_int, [C.c_void_p, C.POINTER(LsqrParams), C.POINTER(LsqrOptions), C.POINTER(TomoReg), _dp, _dp, _dp,
                                         C.POINTER(LsqrStats)]),
    "rtmi_eikonal_tomo_apply_multi": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp, C.POINTER(EikonalTomoStats)]),
    "rtmi_eikonal_tomo_apply_multi_dev": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(EikonalTomoStats)]),
    "rtmi_eikonal_tomo_transpose_multi": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp, C.POINTER(EikonalTomoStats)]),
    "rtmi_eikonal_tomo_transpose_multi_dev": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(EikonalTomoStats)]),
    "rtmi_eikonal_tomo_lsqr_multi": (C.c_int, [C.c_void_p, C.POINTER(LsqrParams), C.POINTER(LsqrOptions), C.POINTER(TomoReg), C.c_int32,
                                               C.c_int32, _dp, _dp, _dp, C.POINTER(LsqrStats)]),
    "rtmi_eikonal_tomo_set_column_group": (C.c_int, [C.c_void_p, C.c_int32]),
    "rtmi_locate_stack": (C.c_int, [C.c_void_p, C.POINTER(StackParams), _dp, _dp, _dp, _ip, _dp, _ip, _dp, C.POINTER(StackEvent),
                                    C.POINTER(C.c_int64), C.POINTER(StackStats)]),
    "rtmi_locate_stack_dev": (C.c_int, [C.c_void_p, C.POINTER(StackParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.POINTER(StackEvent), C.POINTER(C.c_int64), C.POINTER(StackStats)]),
    "rtmi_batch_view": (C.c_int, [C.c_void_p, C.POINTER(DeviceView)]),
    "rtmi_batch_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "rtmi_batch_destroy": (None, [C.c_void_p]),
    "rtmi_shard_create": (C.c_int, [C.c_int] + [C.c_double] * 5 + [C.POINTER(Params), C.c_int64, _dp, _dp, _dp, _ip, C.c_int, C.c_int,
                                    C.POINTER(C.c_void_p)]),
    "rtmi_shard_run": (C.c_int, [C.c_void_p]),
    "rtmi_shard_reset": (C.c_int, [C.c_void_p]),
    "rtmi_shard_read_d_ray": (C.c_int, [C.c_void_p, _dp]),
    "rtmi_shard_read_final": (C.c_int, [C.c_void_p, _dp]),
    "rtmi_shard_gather_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]),
    "rtmi_shard_read_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, _dp]),
    "rtmi_shard_info": (C.c_int, [C.c_void_p, C.POINTER(ShardStats)]),
    "rtmi_shard_batch": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "rtmi_shard_destroy": (None, [C.c_void_p]),
    "rtmi_debug_sincos": (C.c_int, [C.c_int64, _dp, _dp, _dp]),
    "rtmi_debug_arctan2": (C.c_int, [C.c_int64, _dp, _dp, _dp]),
    "rtmi_debug_rcp14_table": (C.c_int, [C.POINTER(C.c_uint16)]),
    "rtmi_debug_exp": (C.c_int, [C.c_int64, _dp, _dp]),
    "rtmi_debug_field_lookup": (C.c_int, [C.c_void_p, C.c_int64] + [_dp] * 5),
    "rtmi_debug_field_lookup_layered": (C.c_int, [C.c_void_p, C.c_int64] + [_dp] * 5),
    "rtmi_field_layered": (C.c_int, [C.c_void_p]),
    "rtmi_debug_auto_rule": (C.c_int, [_dp, C.c_int, _dp, C.c_int, _ip, _ip]),
    "rtmi_debug_paraxial_rows": (C.c_int, [C.c_void_p, _dp, _ip]),
    "rtmi_debug_grid_rows": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [_dp] * 4 + [_ip, _dp, C.POINTER(GridParams), _ip, _dp,
                                                                             C.POINTER(GridStats)]),
    "rtmi_debug_arrival_rows": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [_dp] * 4 + [_ip, _dp, _dp, _ip, _dp, C.POINTER(GridParams),
                                          C.POINTER(ArrivalParams), _ip, _dp, C.POINTER(ArrivalStats)]),
    "rtmi_debug_fix_norm": (C.c_int, [_dp, C.c_int64, _dp, _ip]),
    "rtmi_debug_hilbert": (C.c_int, [_dp, C.c_int64, C.c_int64, _dp, C.c_int32, _dp]),
}

_lib = None


def _share_torchs_hip_runtime():
    """One HIP runtime per process, whatever the import order.

    librtmi.so asks for "libamdhip64.so.7" (RUNPATH /opt/rocm/lib); torch's ROCm wheel bundles a copy of the runtime with the
    same SONAME, and its libraries ask for "libamdhip64.so" -- a name the loader satisfies from an already mapped object only
    when that object is the same FILE.  So: torch first, librtmi second -> librtmi's request matches the SONAME of torch's copy,
    one runtime (fine); librtmi first -> /opt/rocm's copy is mapped, torch later maps its own beside it, and the second HSA
    runtime to open the device is refused ("No HIP GPUs are available"; tools/hip_runtime_probe.py shows both cases).
    Mapping torch's copy (and nothing else of torch) before librtmi.so makes every order the first one: librtmi binds to it by
    SONAME, torch finds the same file when it is imported.  Without torch installed librtmi.so uses /opt/rocm's runtime.
    RTMI_NO_PRELOAD=1 skips this (the probe uses it)."""
    import importlib.util
    import sys
    if os.environ.get("RTMI_NO_PRELOAD"):
        return
    if "torch" in sys.modules:
        # torch imported first: its runtime is mapped once torch has initialised its HIP side; do that before librtmi.so asks
        # for "libamdhip64.so.7", so that the request is answered by SONAME from torch's copy and not from /opt/rocm
        try:
            sys.modules["torch"].cuda.init()
        except Exception:
            pass                                   # no device / a CPU-only torch: librtmi's own calls will say so
        return
    try:
        spec = importlib.util.find_spec("torch")                           # locates the package, does not import it
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    hip = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(hip):
        C.CDLL(hip, mode=C.RTLD_GLOBAL)


def mapped_hip_runtimes():
    """Paths of every libamdhip64 mapped into this process (/proc/self/maps)."""
    found = []
    try:
        with open("/proc/self/maps") as fh:
            for line in fh:
                path = line.rsplit(None, 1)[-1] if "/" in line else ""
                if "libamdhip64" in os.path.basename(path) and path not in found:
                    found.append(path)
    except OSError:
        pass
    return found


def _check_one_hip_runtime():
    """Two HIP runtimes in one process (a torch wheel built for another ROCm major version, so that the SONAMEs differ, or
    RTMI_NO_PRELOAD set) fail much later and far from the cause -- "No HIP GPUs are available" from whichever runtime opens the
    device second.  Say so here, by name, at load time."""
    import warnings
    paths = mapped_hip_runtimes()
    if len({os.path.realpath(p) for p in paths}) > 1:
        msg = ("raytracing_amd: more than one HIP runtime is mapped into this process (" + ", ".join(paths) + "): librtmi.so and "
               "torch would each open the device through their own; the second to do so gets 'No HIP GPUs are available'. "
               "Import raytracing_amd before torch without RTMI_NO_PRELOAD, or use a torch wheel of librtmi's ROCm major version.")
        if os.environ.get("RTMI_STRICT_RUNTIME"):
            raise ImportError(msg)
        warnings.warn(msg, RuntimeWarning, stacklevel=3)


def lib():
    """Load librtmi.so (built in-tree by __graft_entry__.build() / make -C raytracing_amd/csrc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C raytracing_amd/csrc). "
                "raytracing_amd has no CPU fallback.")
        _share_torchs_hip_runtime()
        L = C.CDLL(LIB_PATH)
        _check_one_hip_runtime()
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        if L.rtmi_abi_version() != ABI_VERSION:
            raise ImportError("librtmi.so ABI version mismatch")
        _lib = L
    return _lib


def check(code):
    if code != 0:
        raise RtmiError(code, lib().rtmi_last_error().decode("utf-8", "replace"))


def dptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None
