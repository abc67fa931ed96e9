"""The read-outs of a batch (rows, d_ray, final, metrics, isochrones) in fp32 with sort_rays -- k_unpermute_rows<float> and the
fp32 per-ray pack and metric kernels with a permutation, the one combination test_sort_rays_answers_in_caller_order (fp64) leaves
out -- and at the block boundary of their one-lane-per-ray grids: R = 257 (a full 256-lane block and one lane), 256 and 1.

Every comparison is exact: the recorded rows against the batch's own device arrays un-permuted on the host, the per-ray
read-outs of the sorted batch against the unsorted batch's (a ray's arithmetic does not depend on its slot)."""
import numpy as np
import pytest

from conftest import LIMITS

pytestmark = pytest.mark.gpu

SCEN, METHOD, MAX_SIZE = "vert_heterogeneous", 6, 200


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench
    n = __import__("ctypes").c_int()
    from raytracing_amd import _lib
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


@pytest.fixture(scope="module")
def traced(rb):
    """(dtype name, R) -> the read-outs of the unsorted and the sorted batch, traced once"""
    fields, cache = {}, {}

    def read(F, th, srt, times):
        b = rb.Batch(F, METHOD, rb.DELTA_S, MAX_SIZE, LIMITS[SCEN], 1, th, -2.0, -2.0, record_stride=1, sort_rays=srt,
                     keep_n_ray=True)
        b.run()
        s, n = b.rows(want_n_ray=True)
        if times is None:       # a time every ray reaches, and one between the shortest and the longest ray's last traveltime
            t_end = s[:, 4].max(axis=0)
            times = [0.3 * t_end.min(), 0.5 * (t_end.min() + t_end.max())]
        dt = b.device_tensors()
        out = dict(rows=s, n_ray=n, d_ray=b.d_ray(), final=b.final(), px_cv=b.metric("px_cv"), closure=b.metric("closure"),
                   isochrones=b.isochrones(times), times=times,
                   dev_s=dt["s_ray"].cpu().numpy().astype(np.float64), dev_n=dt["n_ray"].cpu().numpy().astype(np.float64),
                   perm=dt["perm"].cpu().numpy() if "perm" in dt else None)      # copied before the batch (and its memory) goes
        del dt
        b.close()
        return out

    def get(dtype, R):
        if (dtype, R) not in cache:
            if dtype not in fields:
                fields[dtype] = rb.Field.build(SCEN, LIMITS[SCEN], rb.DELTA, rb.F64 if dtype == "f64" else rb.F32)
            th = np.random.default_rng(257).permutation(np.linspace(0.06, np.pi / 2, R))
            plain = read(fields[dtype], th, False, None)
            cache[dtype, R] = (plain, read(fields[dtype], th, True, plain["times"]))
        return cache[dtype, R]
    yield get
    for f in fields.values():
        f.close()


CASES = [("f32", 257), ("f64", 256), ("f64", 1)]


@pytest.mark.parametrize("dtype,R", CASES)
def test_rows_are_the_device_rows_in_caller_order(dtype, R, traced):
    plain, srt = traced(dtype, R)
    assert plain["perm"] is None and sorted(srt["perm"].tolist()) == list(range(R))
    assert plain["rows"].shape == (MAX_SIZE, 6, R) and np.count_nonzero(plain["rows"][-1]) > 0
    for o in (plain, srt):
        perm = np.arange(R) if o["perm"] is None else o["perm"]      # slot k holds the caller's ray perm[k]
        s, n = np.empty_like(o["dev_s"]), np.empty_like(o["dev_n"])
        s[:, :, perm] = o["dev_s"]
        n[:, perm] = o["dev_n"]
        assert np.array_equal(o["rows"], s) and np.array_equal(o["n_ray"], n)


@pytest.mark.parametrize("dtype,R", CASES)
def test_sorted_read_outs_equal_the_unsorted(dtype, R, traced):
    plain, srt = traced(dtype, R)
    assert np.isfinite(plain["isochrones"]).any() and (R == 1 or np.isnan(plain["isochrones"]).any())
    for k in ("d_ray", "final", "px_cv", "closure", "isochrones", "rows", "n_ray"):
        assert np.array_equal(plain[k], srt[k], equal_nan=True), k
