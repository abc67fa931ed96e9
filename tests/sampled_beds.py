"""Small seeded test beds on caller-sampled fields (Field.from_samples), for the step methods and the post-trace kernels at the
edges of the grid: unpadded grids whose boxes reach past them, so that recorded rows lie in the not-a-knot rim cells and off the
grid (FITPACK's argument clamp), unequal spacings, plateaus of exactly equal samples, ragged batch sizes.  Test infrastructure.

Each bed is (x, y, Z, delta, box) with a step, a max_size that truncates some rays and a receiver line that runs partly off the
grid; Bed.launches gives the seeded launch points and directions of a ragged batch."""
import numpy as np

RAGGED = (1, 63, 65, 333)      # batch sizes around one and two 64-lane waves, and a tail wave one third full


class Bed:
    def __init__(self, name, x, y, Z, delta, box, step, max_size, line):
        self.name = name
        self.x = np.asarray(x, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64)
        self.Z = np.ascontiguousarray(Z, dtype=np.float64)
        self.delta, self.box, self.step, self.max_size = float(delta), tuple(float(v) for v in box), float(step), int(max_size)
        self.line = line

    def __repr__(self):
        return self.name

    def fields(self):
        """(x, y, Z, delta, box)"""
        return self.x, self.y, self.Z, self.delta, self.box

    def off_grid(self, px, py):
        px, py = np.asarray(px), np.asarray(py)
        return (px < self.x[0]) | (px > self.x[-1]) | (py < self.y[0]) | (py > self.y[-1])

    def in_rim(self, px, py):
        """On the grid, in the first two or last two cells of an axis: the not-a-knot end intervals of the bicubic fits."""
        px, py = np.asarray(px), np.asarray(py)

        def rim(p, a):
            return ((p >= a[0]) & (p < a[2])) | ((p > a[-3]) & (p <= a[-1]))
        return ~self.off_grid(px, py) & (rim(px, self.x) | rim(py, self.y))

    def edge_counts(self, s_ray, last):
        """(rows off the grid, rows in rim cells) among the recorded rows 0 .. last of every ray"""
        s_ray = np.asarray(s_ray)
        last = np.minimum(np.asarray(last, dtype=np.int64), s_ray.shape[0] - 1)
        live = np.arange(s_ray.shape[0])[:, None] <= last[None, :]
        px, py = s_ray[:, 0][live], s_ray[:, 1][live]
        return int(self.off_grid(px, py).sum()), int(self.in_rim(px, py).sum())

    def launches(self, R, seed):
        """x0, y0, theta [R]: starts anywhere in the box (some off the grid), directions uniform in (-pi, pi]; in batches of
        3 rays or more, rays 1, R // 2 and R - 1 start outside the box (they stop after one step)."""
        rng = np.random.default_rng(seed)
        xi, xs, yi, ys = self.box
        x0 = rng.uniform(xi, xs, R)
        y0 = rng.uniform(yi, ys, R)
        th = np.pi - rng.uniform(0.0, 2.0 * np.pi, R)
        if R >= 3:
            out = np.array([1, R // 2, R - 1])
            x0[out] = (xi - 0.25, xs + 0.5, 0.5 * (xi + xs))
            y0[out] = (0.5 * (yi + ys), 0.5 * (yi + ys), ys + 0.75)
        return x0, y0, th

    def fan(self, R, source):
        """R launch angles in (-pi, pi], in order, from one source: a fan for first_arrival_grid"""
        return np.pi - (np.arange(R) + 0.5) * (2.0 * np.pi / R), source[0], source[1]


def _rim8():
    x = np.linspace(-1.0, 2.0, 8); y = np.linspace(0.5, 2.5, 8)
    X, Y = np.meshgrid(x, y)
    Z = 1.3 + 0.25 * np.sin(1.1 * X + 0.3) * np.cos(0.9 * Y) + 0.1 * np.abs(X - 0.4)   # test_cell_polynomials_on_arbitrary_grids'
    delta = 0.5 * ((x[1] - x[0]) + (y[1] - y[0]))
    return Bed("rim8", x, y, Z, delta, (-2.0, 3.0, -0.5, 3.5), 0.02, 200, (0.0, 1.0, 1.6))


def _thin():
    x = np.linspace(0.0, 3.0, 64); y = np.linspace(0.0, 2.0, 11)           # hx / hy = 0.238
    X, Y = np.meshgrid(x, y)
    Z = 1.2 + 0.2 * np.sin(1.7 * X) * np.cos(1.3 * Y + 0.2) + 0.05 * X * Y
    delta = 0.5 * ((x[1] - x[0]) + (y[1] - y[0]))
    return Bed("thin", x, y, Z, delta, (0.01, 3.6, -0.6, 1.99), 0.01, 300, (0.0, 1.0, 0.9))   # box past x = 3 and y = 0 only


def _layers():
    x = np.linspace(-1.0, 1.0, 25); y = np.linspace(0.0, 2.0, 65)
    n = np.where(y < 0.6, 1.0, np.where(y < 1.3, 1.25, 1.5))              # three horizontal layers, equal samples in each
    Z = np.broadcast_to(n[:, None], (len(y), len(x))).copy()
    return Bed("layers", x, y, Z, y[1] - y[0], (-1.5, 1.5, -0.5, 2.5), 0.01, 260, (1.0, 0.0, 0.3))


def _const():
    x = np.linspace(0.0, 1.0, 8); y = np.linspace(0.0, 1.0, 8)
    Z = np.full((8, 8), 1.5)
    return Bed("const", x, y, Z, x[1] - x[0], (-3.0, 4.0, -3.0, 4.0), 0.02, 300, (0.0, 1.0, 0.5))


BEDS = {b.name: b for b in (_rim8(), _thin(), _layers(), _const())}
