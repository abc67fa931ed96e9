"""GPU: the checks every entry that reads a batch's recorded trajectory makes before it touches the rows (the shared preamble of
raytracing_amd/csrc/rtmi_host.h), entry by entry.  A batch recorded with a stride is refused by all of them (-1, under the
entry's own name); a batch whose rows were continued from rtmi_batch_set_state is refused (-4) by the entries that need a
trajectory from the launch point, and read as it is by the others.  Refusals on the host: no kernel runs."""
import numpy as np
import pytest

from conftest import LIMITS

pytestmark = pytest.mark.gpu

GRID = (-1.95, 0.05, 140, -2.45, 0.05, 70)
LINE = (1.0, 0.0, 1.0)
TIMES = [2.0, 4.0]

# entry -> (the C entry that reports, the call, the code after get_state / set_state at the current row).  The codes are the
# library's behaviour before the preamble was shared: crossings, isochrones and wavefronts read rows wherever they came from.
ENTRIES = {
    "crossings": ("rtmi_crossings", lambda b: b.crossings(LINE), 0),
    "paraxial": ("rtmi_paraxial", lambda b: b.paraxial(), -4),
    "paraxial_rows": ("rtmi_debug_paraxial_rows", lambda b: b.paraxial_rows(), -4),
    "first_arrival_grid": ("rtmi_first_arrival_grid", lambda b: b.first_arrival_grid(GRID), -4),
    "gaussian_beams": ("rtmi_gaussian_beams", lambda b: b.gaussian_beams(GRID, [20.0], 1.0), -4),
    "traveltime_perturb": ("rtmi_traveltime_perturb", lambda b: b.traveltime_perturb(np.zeros((b.field.qy, b.field.qx))), -4),
    "traveltime_backproject": ("rtmi_traveltime_backproject", lambda b: b.traveltime_backproject(w_end=np.ones(b.R)), -4),
    "isochrones": ("rtmi_isochrones", lambda b: b.isochrones(TIMES), 0),
    "wavefronts": ("rtmi_wavefronts", lambda b: b.wavefronts(TIMES), 0),
}


def _code(call, b):
    from raytracing_amd import _lib
    try:
        call(b)
    except _lib.RtmiError as e:
        return e.code, str(e)
    return 0, ""


def test_every_entry_checks_the_record_before_it_reads_it():
    from raytracing_amd import rt_bench as rb
    F = rb.Field.build("vert_heterogeneous", LIMITS["vert_heterogeneous"], rb.DELTA)
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    th = np.linspace(0.05, np.pi / 2 - 0.05, 64)

    def batch(**kw):
        b = rb.Batch(F, rb.op6, rb.DELTA_S, ms, LIMITS["vert_heterogeneous"], 1, th, -2.0, -2.0, keep_n_ray=False, **kw)
        b.run()
        return b

    # (a) a strided record
    b = batch(record_stride=4)
    for name, (entry, call, _) in ENTRIES.items():
        code, msg = _code(call, b)
        assert code == -1, (name, code, msg)
        assert msg.startswith(f"librtmi error -1: {entry}: ") and "record_stride" in msg, (name, msg)
    b.close()
    # (b) rows continued from a caller-set state at the current row
    b = batch()
    st, aux, ist, al = b.get_state()
    b.set_state(st, istep=ist)
    for name, (entry, call, want) in ENTRIES.items():
        code, msg = _code(call, b)
        assert code == want, (name, code, msg)
        if want:
            assert msg.startswith(f"librtmi error {want}: {entry}: ") and "set_state" in msg, (name, msg)
    b.close()
    F.close()


def test_isochrones_and_wavefronts_refuse_another_device():
    """With another device current, the per-ray stage refuses the batch before it asks for its rows: both entries report it under
    rtmi_isochrones' name (-1).  Needs two GPUs."""
    import ctypes as C
    from raytracing_amd import _lib
    from raytracing_amd import rt_bench as rb
    n = C.c_int(0)
    _lib.check(_lib.lib().rtmi_device_count(C.byref(n)))
    if n.value < 2:
        pytest.skip(f"needs 2 GPUs, this host has {n.value}")
    _lib.check(_lib.lib().rtmi_set_device(0))
    F = rb.Field.build("vert_heterogeneous", LIMITS["vert_heterogeneous"], rb.DELTA)
    ms = int(np.ceil(80 / rb.DELTA_S) + 1)
    th = np.linspace(0.05, np.pi / 2 - 0.05, 64)
    b = rb.Batch(F, rb.op6, rb.DELTA_S, ms, LIMITS["vert_heterogeneous"], 1, th, -2.0, -2.0, keep_n_ray=False)
    b.run()
    try:
        _lib.check(_lib.lib().rtmi_set_device(1))
        for name in ("isochrones", "wavefronts"):
            code, msg = _code(ENTRIES[name][1], b)
            assert code == -1, (name, code, msg)
            assert msg.startswith("librtmi error -1: rtmi_isochrones: the field lives on device"), (name, msg)
    finally:
        _lib.check(_lib.lib().rtmi_set_device(0))
    b.close()
    F.close()
