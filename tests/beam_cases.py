"""The Gaussian-beam cases in which the tiles, the cap max_width, the cutoff, the frequency groups of 8 and the record's length
decide something, and the conditions that make each worth running.  tests/test_beam_ref.py asserts the conditions on the
oracle's rows, tests/test_gpu_beam_edges.py on the device's rows before it compares the device with the restatement
(tests/beam_ref.py).  Test infrastructure.

The conditions are properties of the inputs, not measurements: if one fails, the input changes, not the condition."""
import numpy as np

import beam_ref as B

SCENARIO = "vert_heterogeneous"
METHOD = 6
STEP_MULT = 4                                  # step = 4 DELTA_S
LENGTH = 8.0                                   # max_size = ceil(LENGTH / step) + 1
SOURCE = (-2.0, -2.0)
FAN = (0.05, np.pi / 2 - 0.05)
RAYS = 32
EPS = 28.0
THREE_SOURCES = ((-2.0, -2.0), (-1.5, -2.2), (-1.0, -1.8))

G1 = (-1.95, 0.05, 50, -2.45, 0.07, 37)        # 4 x 3 tiles of 0.8 x 1.12, ragged last tiles, gdx != gdy
OM17 = tuple(np.linspace(300.0, 900.0, 17)[::-1])

# id -> grid, omegas, the beam parameters, and optionally rec_rows and sources
CASES = {
    "cap_narrow": dict(grid=G1, om=(300.0, 700.0), kw=dict(max_width=0.12)),
    "cap_wide": dict(grid=G1, om=(300.0, 700.0), kw=dict(max_width=0.5)),
    "cutoff_small": dict(grid=G1, om=(300.0, 1200.0), kw=dict(cutoff=3.0)),
    "omin_not_first": dict(grid=G1, om=(700.0, 300.0, 1200.0), kw=dict(cutoff=3.0, max_width=0.5)),
    "nw17_col1": dict(grid=(-1.9, 0.1, 17, -2.4, 0.1, 16), om=OM17, kw=dict(max_width=0.4)),
    "nw9_row1": dict(grid=(-1.9, 0.1, 16, -2.4, 0.1, 17), om=OM17[:9], kw=dict(max_width=0.4)),
    "nw8": dict(grid=(-1.9, 0.1, 16, -2.4, 0.1, 17), om=OM17[:8], kw=dict(max_width=0.4)),
    "flat_wide": dict(grid=(-1.9, 0.06, 33, -2.3, 0.3, 5), om=(300.0, 700.0), kw=dict(max_width=0.4)),
    "line": dict(grid=(-1.0, 0.03, 1, -2.4, 0.03, 40), om=(300.0, 700.0), kw=dict(max_width=0.3)),
    "one_node": dict(grid=(-1.9, 0.1, 1, -2.3, 0.1, 1), om=(300.0, 700.0), kw=dict(max_width=0.4)),
    "off_grid": dict(grid=(5.5, 0.1, 20, 1.5, 0.1, 20), om=(300.0,), kw=dict(max_width=0.2)),
    "taper": dict(grid=G1, om=(300.0, 700.0), kw=dict(edge_taper=0.3)),
    "short_record": dict(grid=(-1.95, 0.1, 50, -2.45, 0.07, 37), om=(300.0, 700.0), kw=dict(max_width=0.5), rec_rows=320),
    "three_sources": dict(grid=G1, om=(300.0, 700.0), kw=dict(max_width=0.5), sources=THREE_SOURCES),
}
G1_CASES = [k for k, c in CASES.items() if c["grid"] == G1 and "sources" not in c]


def fan_params(delta_s):
    """(step, max_size) of the common fan"""
    step = STEP_MULT * delta_s
    return step, int(np.ceil(LENGTH / step)) + 1


def launch(case):
    """theta0, x0, y0 [R] and fan_size of a case: every source launches the same fan"""
    src = np.array(CASES[case].get("sources", (SOURCE,)))
    th = np.linspace(FAN[0], FAN[1], RAYS)
    return np.tile(th, len(src)), np.repeat(src[:, 0], RAYS), np.repeat(src[:, 1], RAYS), RAYS


def restate(case, s_ray, last, field, theta0, counts=None, tube=None, **over):
    """the restatement of a case on the given rows; over replaces beam parameters"""
    c = CASES[case]
    kw = dict(c["kw"], **over)
    return B.gaussian_beams(s_ray, last, field, theta0, RAYS, c["grid"], c["om"], EPS, tube=tube, counts=counts, **kw)


def rel_change(a, b):
    """max |a - b| / max |b| over everything"""
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def check_binds(case, u, cn, last_raw=None, u_full=None, u_plain=None):
    """Assert that the case binds what it is there for.  u, cn: the restatement's field and counts; last_raw: every ray's last
    written row (short_record); u_full: the restatement on the full record (short_record); u_plain: without the taper (taper)."""
    c = CASES[case]
    if case in G1_CASES or case == "three_sources":
        assert cn["inside"] >= 1000
    if case == "one_node":
        assert cn["inside"] >= 1
    if case == "line":
        assert cn["inside"] >= 100
    if "max_width" in c["kw"]:
        assert cn["capped"] == cn["segments"]
    if case == "cutoff_small":
        assert cn["capped"] == 0
        assert c["om"][-1] == max(c["om"])
        assert cn["inside_per_omega"][-1] <= 0.7 * cn["inside"]
    if case == "omin_not_first":
        assert int(np.argmin(c["om"])) != 0
        assert cn["inside_per_omega"][int(np.argmin(c["om"]))] == cn["inside"]
    if case in ("nw17_col1", "nw9_row1", "nw8"):
        nw, g = len(c["om"]), c["grid"]
        assert nw == {"nw17_col1": 17, "nw9_row1": 9, "nw8": 8}[case]
        assert case != "nw17_col1" or (int(np.argmin(c["om"])) == 16 and g[2] % 16 == 1)      # 8 + 8 + 1, omega_min in the last
        assert case == "nw17_col1" or g[5] % 16 == 1
        assert cn["inside"] >= 1000
    if case == "off_grid":
        # a step's wedge reaches any distance, so far nodes can be owned; none is within q_max, which is what the tiles prune by
        assert cn["inside"] == 0 and not u.any()
    if case == "short_record":
        rr = c["rec_rows"]
        assert int((last_raw > rr - 1).sum()) >= 5 and int((last_raw < rr - 1).sum()) >= 5
        assert np.mean(u != u_full) >= 0.10
    if case == "taper":
        assert rel_change(u, u_plain) >= 0.05
    assert cn["near"] * 10000 <= cn["inside"]
    assert cn["inside"] <= cn["owned"] and np.isfinite(u).all()
