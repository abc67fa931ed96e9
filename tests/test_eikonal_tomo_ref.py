"""CPU: the restatement of first-arrival eikonal tomography (tests/eikonal_tomo_ref.py) on its own: the
cell weights against the functions that exist, the sample where the clip of i0 fires, the adjointness of the two products in exact
arithmetic, dead and live rows behind walls, the operator against the dense Jacobian of section 35, and one damped step of
tomography with the receivers off the nodes."""
from fractions import Fraction

import numpy as np

import eikonal_lin_ref as L
import eikonal_ref as R
import eikonal_tomo_ref as E
from raytracing_amd import rt_bench

ADJOINT_BOUND = 2e-16       # measured 1.7e-16 on the case below


def test_cell_weights_are_those_of_the_functions_that_exist():
    grid, _, _, src, _, idx, w = L.tomography_case()
    ridx, rw, inside = E.cells(grid, src, source=True)
    assert inside.all() and np.array_equal(ridx, idx) and R.same_bits(rw, w)
    rng = np.random.default_rng(3)
    for g in (grid, (0.5, 0.25, 1, -1.0, 0.2, 9), (0.5, 0.25, 9, -1.0, 0.2, 1), (0.0, 1.0, 1, 0.0, 1.0, 1)):
        gx0, gdx, nx, gy0, gdy, ny = g
        pts = np.array([E.at(g, u, v) for u, v in rng.uniform(-0.5, 1.5, (60, 2)) * [nx - 1, ny - 1]] + [E.at(g, nx - 1.0, ny - 1.0), E.at(g, 0, 0)] +
                       [[gx0 - 0.5 * gdx, gy0], [gx0, gy0 + ny * gdy], [gx0 + (nx + 3) * gdx, gy0 - 2 * gdy]])
        bidx, bw = rt_bench.eikonal_source_weights(pts, g)
        ridx, rw, inside = E.cells(g, pts, source=True)
        assert np.array_equal(ridx, bidx) and R.same_bits(rw, bw + 0.0)           # + 0.0: the product with False may give -0.0
        assert (~inside).sum() == 3 and not rw[~inside].any() and not np.signbit(rw[~inside]).any()
        if nx > 1 and ny > 1:                                                      # eikonal_lin_ref's is for grids with cells
            lidx, lw = L.source_weights(pts[inside], g)
            assert np.array_equal(ridx[inside], lidx) and R.same_bits(rw[inside], lw)


def test_sample_at_a_node_on_an_edge_and_where_the_clip_fires():
    g = (-1.0, 0.5, 5, 2.0, 0.25, 4)
    X, Y = R.nodes(g)
    f = (3.0 + 2.0 * X - 5.0 * Y).reshape(-1)                                      # bilinear interpolation is exact on it
    for (u, v), corners, weights in (((2.0, 1.0), [7, 8, 12, 13], [1.0, 0.0, 0.0, 0.0]),          # a node
                                     ((2.5, 1.0), [7, 8, 12, 13], [0.5, 0.5, 0.0, 0.0]),          # an edge
                                     ((4.0, 1.5), [8, 9, 13, 14], [0.0, 0.5, 0.0, 0.5]),          # the last column: i0 = nx - 2, fu = 1
                                     ((1.25, 3.0), [11, 12, 16, 17], [0.0, 0.0, 0.75, 0.25]),     # the last row: j0 = ny - 2, fv = 1
                                     ((4.0, 3.0), [13, 14, 18, 19], [0.0, 0.0, 0.0, 1.0])):       # the far corner
        x, y = E.at(g, u, v)
        idx, w, inside = E.cell(g, x, y)
        assert inside and idx == corners and w == weights
        assert E.sample(f, idx, w) == 3.0 + 2.0 * x - 5.0 * y
    idx, w, _ = E.cell((0.0, 1.0, 1, 0.0, 1.0, 3), 0.0, 1.5)                       # one column: both x corners are the node
    assert idx == [1, 1, 2, 2] and w == [0.5, 0.0, 0.5, 0.0]
    assert E.sample([1.0, 2.0, 4.0], idx, w) == 3.0


def test_the_two_products_are_adjoint_in_exact_arithmetic():
    grid = L.GRADIENT_GRID
    rec = np.array([E.at(grid, u, v) for u, v in [(10.3, 5.7), (33.5, 20.25), (40.2, 40.6), (40.7, 40.1), (69.5, 55.5), (5.0, 50.0), (60.25, 3.0)]])
    op = E.operator(L.gradient_case(), rec)
    assert op.live.all() and op.inside.all()
    assert len({tuple(op.ridx[2]), tuple(op.ridx[3])}) == 1                         # two receivers in one cell
    rng = np.random.default_rng(7)
    v, u = rng.standard_normal(op.nn), rng.standard_normal(op.S * op.R)
    Av, Atu = op.apply(v), op.transpose(u)
    lhs = sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(Av, u))
    rhs = sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(v, Atu))
    rel = float(abs(lhs - rhs) / abs(lhs))
    print(f"<A v, u> = {float(lhs):.17g}, relative difference to <v, A^T u> {rel:.2e}")
    assert rel <= ADJOINT_BOUND


def test_dead_and_live_rows_behind_walls():
    grid, n, src, ns, fill, rec, op = E.walls()
    assert op.live.shape == (2, len(rec))
    assert list(op.live_per) == [5, 5] and list((~op.live).sum(axis=1)) == [3, 3]
    assert not op.live[:, [0, 1, 4]].any()                  # a corner with n = inf, the sealed pocket, a corner with n = 0
    rng = np.random.default_rng(5)
    y = op.apply(rng.standard_normal(op.nn))
    assert not y.reshape(2, -1)[~op.live].any() and y.reshape(2, -1)[op.live].all()
    u = rng.standard_normal(op.S * op.R)
    planted = u.copy()
    planted[~op.live.reshape(-1)] = np.nan                  # the transpose does not read a dead row's entry
    assert R.same_bits(op.transpose(u), op.transpose(planted)) and np.isfinite(op.transpose(planted)).all()
    picks = rng.standard_normal(op.S * op.R)
    picks[2] = np.nan
    res = op.residual(picks)
    assert not res[~op.live.reshape(-1)].any() and res[2] == 0.0 and not np.signbit(res[2]) and res[3] != 0.0


def test_on_nodes_with_one_source_outside_the_operator_is_a_row_selection_of_the_dense_jacobian():
    grid = (0.5, 0.25, 13, -1.0, 0.125, 11)                                         # spacings that put a receiver on a node exactly
    X, Y = R.nodes(grid)
    n = 1.0 + 0.25 * np.sin(1.3 * X + 0.4) * np.cos(0.9 * Y - 0.2)
    src = np.array([[0.5 - 0.6 * 0.25, -1.0 + 2.3 * 0.125]])
    ns = np.array([1.1])
    fill = R.solve(grid, n, src, ns)
    nodes = [0, 5, 12, 40, 77, 13 * 10 + 12, 13 * 10, 64]                           # corners, the last column and row included
    rec = np.array([[0.5 + (x % 13) * 0.25, -1.0 + (x // 13) * 0.125] for x in nodes])
    op = E.Operator(grid, n, src, ns, fill, rec)
    assert not op.inside.any() and op.live.all() and sorted(op.rw.reshape(-1))[-9:] == [0.0] + [1.0] * 8
    J = L.dense_jacobian(op.nets, nodes, np.zeros((1, 4), dtype=np.int64), np.zeros((1, 4)))
    assert R.same_bits(op.dense(), J + 0.0) and np.abs(J).sum() > 0


def solve_tables(n, ns):
    grid, _, _, src, _, _, _ = L.tomography_case()
    fill = R.solve(grid, n, src, ns)
    return fill["T"], (n, ns, fill)


def test_one_damped_step_with_the_receivers_off_the_nodes():
    grid, _, _, src, _, _, _ = L.tomography_case()
    pts = E.tomography_receivers()
    assert all(E.receiver_ok(grid, x, y) for x, y in pts) and all(max(E.cell(grid, x, y)[1]) < 0.75 for x, y in pts)

    def jacobian(state):
        n, ns, fill = state
        return E.Operator(grid, n, src, ns, fill, pts).dense_by_nodes()
    r0, r1, step = L.tomography_step(*E.tomography_hooks(solve_tables, jacobian))
    print(f"off-node tomography step: rms residual {r0:.6e} -> {r1:.6e}, fraction {r1 / r0:.4f}")
    assert r1 <= E.TOMO_BOUND * r0 and np.abs(step).max() > 0
