"""GPU: rtmi_gaussian_beams where its machinery decides something (tests/beam_cases.py): footprints narrower than a tile, ragged
and one-node-wide last tiles, a receiver line, a single node, gdx != gdy, a grid no step reaches, max_width, cutoff and edge_taper
off their defaults, 8, 9 and 17 frequencies with the lowest one anywhere, a record shorter than its rays, three sources, fp32
records on their own rows, a fan without steps.  Every case first asserts on the device's rows the conditions that
tests/test_beam_ref.py asserts on the oracle's, then holds the device to the numpy restatement (tests/beam_ref.py) of the same
rows: the values, the exact zeros, and the stats' counts against the restatement's, which tests every (step, node) pair and so
owes nothing to the binning.  Measured numbers are in DESIGN.md section 13."""
import numpy as np
import pytest

import beam_cases as BC
import beam_ref as B
import paraxial_ref as P
from conftest import LIMITS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = __import__("ctypes").c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


@pytest.fixture(scope="module")
def fields(rb):
    cache = {}

    def get(dtype=0):
        if dtype not in cache:
            F = rb.Field.build(BC.SCENARIO, LIMITS[BC.SCENARIO], rb.DELTA, dtype=dtype)
            cache[dtype] = (F, P.SplineField(*F.arrays()))
        return cache[dtype]
    yield get
    for F, _ in cache.values():
        F.close()


@pytest.fixture(scope="module")
def fans(rb, fields):
    """the traced fan of a case, shared by the cases with the same sources, record and dtype: the batch, its rows, every ray's
    last written row, the launch angles and the restatement's tube on those rows"""
    cache = {}

    def get(case, dtype=0, **batch_kw):
        c = BC.CASES[case]
        key = (c.get("sources"), c.get("rec_rows"), dtype, tuple(sorted(batch_kw.items())))
        if key not in cache:
            F, S = fields(dtype)
            step, ms = BC.fan_params(rb.DELTA_S)
            th, x0, y0, _ = BC.launch(case)
            b = rb.Batch(F, rb.METHODS[BC.METHOD], step, ms, LIMITS[BC.SCENARIO], 1, th, x0, y0, rec_rows=c.get("rec_rows", 0),
                         keep_n_ray=False, **batch_kw)
            b.run()
            rows, last = b.rows(), b.d_ray()[2].astype(np.int64)
            cache[key] = (b, rows, last, S, th, B.tube_rows(rows, last, S))
        return cache[key]
    yield get
    for b, *_ in cache.values():
        b.close()


def beams(b, case, om=None, **over):
    c = BC.CASES[case]
    om = c["om"] if om is None else om
    return b.gaussian_beams(c["grid"], om, BC.EPS, fan_size=BC.RAYS, stats=True, **dict(c["kw"], **over))


def bits(u):
    return np.ascontiguousarray(u).view(np.uint64)


def rel_to_max(a, b):
    """per source and frequency: max |a - b| / max |b|, the largest of them"""
    return max(float(np.max(np.abs(a[s, q] - b[s, q])) / np.max(np.abs(b[s, q])))
               for s in range(a.shape[0]) for q in range(a.shape[1]))


def against_the_restatement(case, u, st, ref, cn, bound=1e-10, exact_counts=True):
    """items 1 to 4: values, exact zeros, nothing missed or invented, stats"""
    c = BC.CASES[case]
    assert np.isfinite(u).all()
    err = rel_to_max(u, ref) if np.abs(ref).max() > 0 else 0.0
    zeros = ref == 0
    print(f"{case}: error {err:.2e} of max|u| {np.abs(ref).max():.3e}; {int(zeros.sum())} of {ref.size} outputs exactly 0; "
          f"restatement {cn}; device {st}")
    assert err <= bound
    assert not bits(u[zeros]).any()                    # exactly 0 in both parts (the wrapper's re + 1j im shows no sign of zero)
    if exact_counts:
        if "max_width" in c["kw"]:
            assert cn["near"] == 0                     # q_max is the constant itself: no threshold depends on a device-only value
        assert abs(st["pairs_inside"] - cn["inside"]) <= cn["near"]
    assert st["segments"] == cn["segments"] and st["capped"] == cn["capped"]
    assert cn["inside"] <= st["pairs_tested"] <= 256 * st["tile_entries"]
    if case == "cap_narrow":
        # the footprint box is at most 2 (0.12 + chord) + chord wide, narrower than a tile in both axes: two tile indices per axis
        assert st["tile_entries"] <= 4 * st["segments"]
    if case == "off_grid":
        assert st["tile_entries"] == 0 and st["pairs_tested"] == 0 and st["pairs_inside"] == 0
    gdx, gdy = c["grid"][1], c["grid"][4]
    assert st["max_width"] == c["kw"].get("max_width", B.WIDTH_CELLS * max(gdx, gdy))
    assert st["cutoff"] == c["kw"].get("cutoff", B.CUTOFF)


SINGLE = [k for k in BC.CASES if k != "three_sources"]


@pytest.mark.parametrize("case", SINGLE)
def test_device_equals_the_restatement_where_the_machinery_binds(rb, fans, case):
    b, rows, last, S, th, tube = fans(case)
    u, st = beams(b, case)
    cn, extra = {}, {}
    ref = BC.restate(case, rows, last, S, th, counts=cn, tube=tube)
    if case == "short_record":
        bf, rows_f, last_f, _, _, tube_f = fans("cap_wide")
        extra = dict(last_raw=last, u_full=BC.restate(case, rows_f, last_f, S, th, tube=tube_f))
    if case == "taper":
        extra = dict(u_plain=BC.restate(case, rows, last, S, th, tube=tube, edge_taper=0.0))
    BC.check_binds(case, ref, cn, **extra)
    against_the_restatement(case, u, st, ref, cn)
    if case == "short_record":                         # a different answer from the full record's, on the device too
        full, _ = beams(bf, case)
        differ = float(np.mean(full != u))
        print(f"short_record: {differ:.3f} of the outputs differ from the full record's")
        assert differ >= 0.10
    if case == "nw17_col1":                            # the frequency groups carry no state: any order, the same planes
        perm = np.random.default_rng(17).permutation(17)
        assert not np.array_equal(perm // 8, np.arange(17) // 8)
        u2, _ = beams(b, case, om=np.asarray(BC.CASES[case]["om"])[perm])
        assert np.array_equal(bits(u2), bits(u[:, perm]))


def test_three_sources_equal_the_restatement_in_two_schedules(rb, fans):
    case = "three_sources"
    b, rows, last, S, th, tube = fans(case, sort_rays=False, launch_mode="plain")
    u, st = beams(b, case)
    cn = {}
    ref = BC.restate(case, rows, last, S, th, counts=cn, tube=tube)
    BC.check_binds(case, ref, cn)
    against_the_restatement(case, u, st, ref, cn)
    assert u.shape[0] == 3 and all(np.abs(ref[s]).max() > 0 for s in range(3))
    assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(ref[1], ref[2])
    b2 = fans(case, sort_rays=True, launch_mode="sliced")[0]
    u2, st2 = beams(b2, case)
    assert np.array_equal(bits(u2), bits(u))
    assert all(st2[k] == st[k] for k in ("segments", "tile_entries", "pairs_tested", "pairs_inside", "capped"))


def test_a_fan_without_steps_gives_zeros(rb, fields):
    """A batch that has not stepped holds row 0 alone of every ray: no steps, no tile entries, nothing to scan or sort, and the
    call succeeds with u exactly 0.  (A source outside the box still takes the one step that finds it outside, so after run()
    there are 16 steps, all far from the grid.)"""
    F, _ = fields()
    step, ms = BC.fan_params(rb.DELTA_S)
    th = np.linspace(BC.FAN[0], BC.FAN[1], 16)
    b = rb.Batch(F, rb.METHODS[BC.METHOD], step, ms, LIMITS[BC.SCENARIO], 1, th, 9.0, 9.0, keep_n_ray=False)
    for segments in (0, 16):
        assert int(b.d_ray()[2].sum()) == segments
        u, st = b.gaussian_beams(BC.G1, (300.0, 700.0), BC.EPS, stats=True)       # return code 0: the wrapper raises otherwise
        print(f"{segments} steps: stats {st}")
        assert u.shape == (1, 2, 37, 50) and not bits(u).any()
        assert st["segments"] == segments and st["capped"] == 0
        assert st["tile_entries"] == 0 and st["pairs_tested"] == 0 and st["pairs_inside"] == 0
        b.run()
    b.close()


# fp32 records: the rows, the field's samples and rtmi_paraxial's lookups are fp32, everything after them fp64.  The restatement
# takes the same fp32 rows, widened, but looks the field up in fp64 splines of the fp32 samples.  Measured on MI355X: 2.2e-8 of
# max|u|; the bound is ten times that, rounded up to a power of ten.  The margin is for the other
# arctan2 / exp / sincos libraries and for pairs near the cutoff, which fp32 lookups may move across it.
FP32_BOUND = 1e-6


def test_fp32_records_against_the_restatement_on_their_own_rows(rb, fans):
    case = "cap_wide"
    b, rows, last, S, th, tube = fans(case, dtype=1)
    u, st = beams(b, case)
    cn = {}
    ref = BC.restate(case, rows, last, S, th, counts=cn, tube=tube)
    BC.check_binds(case, ref, cn)
    err = rel_to_max(u, ref)
    print(f"fp32 records on their own rows: {err:.3e}; inside {st['pairs_inside']} against {cn['inside']}")
    against_the_restatement(case, u, st, ref, cn, bound=FP32_BOUND, exact_counts=False)


def test_same_bits_twice_under_the_cap(rb, fans):
    b = fans("cap_narrow")[0]
    u1, st1 = beams(b, "cap_narrow")
    u2, st2 = beams(b, "cap_narrow")
    assert np.abs(u1).max() > 0
    assert np.array_equal(bits(u1), bits(u2))
    assert all(st1[k] == st2[k] for k in ("segments", "tile_entries", "pairs_tested", "pairs_inside", "capped"))
