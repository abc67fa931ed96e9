"""bench.py --dump-outputs: what the timed path's last pass returned, on a fixed sample of rays, within 64 MB.  CPU: the
sampling and the files, on a stand-in for rt_bench.Batch whose "device" tensors are CPU tensors; GPU: bench.py itself."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


class FakeBatch:
    """d_ray, final and the record of R rays, every value naming its ray; the record in slot order perm like a sort_rays batch."""

    def __init__(self, R, rows, dtype=torch.float64, perm=None, n_ray=False, lazy=False):
        self.R = R
        k = np.arange(R, dtype=np.float64)
        self._d = np.stack([k + 0.25 * j for j in range(3)])
        self._f = np.stack([k + 0.5 * j for j in range(9)])
        self._t = {}
        if lazy:                                          # the bench's own size, without its memory: a broadcast view
            self._t["s_ray"] = torch.zeros((), dtype=dtype).expand(rows, 6, R)
            return
        caller = torch.arange(R, dtype=torch.float64) if perm is None else torch.from_numpy(perm).double()
        rec = caller[None, None, :] + 1e-3 * torch.arange(rows, dtype=torch.float64)[:, None, None] \
            + 1e-5 * torch.arange(6, dtype=torch.float64)[None, :, None]
        self._t["s_ray"] = rec.to(dtype)
        if n_ray:
            self._t["n_ray"] = (caller[None, :] + 1e-3 * torch.arange(rows, dtype=torch.float64)[:, None]).to(dtype)
        if perm is not None:
            self._t["perm"] = torch.from_numpy(perm.astype(np.int32))

    def d_ray(self):
        return self._d.copy()

    def final(self):
        return self._f.copy()

    def device_tensors(self):
        return dict(self._t)


def _load(d):
    return {fn[:-4]: np.load(os.path.join(d, fn)) for fn in sorted(os.listdir(d))}


def _bytes(d):
    return sum(os.path.getsize(os.path.join(d, fn)) for fn in os.listdir(d))


def test_dump_is_the_callers_rays_in_the_callers_order(monkeypatch, tmp_path):
    monkeypatch.setattr(bench, "DUMP_RAYS", 1000)
    monkeypatch.setattr(bench, "DUMP_BYTES", 400_000)
    R, rows = 5000, 40
    perm = np.random.default_rng(7).permutation(R)
    bench.dump_outputs(FakeBatch(R, rows, perm=perm, n_ray=True), str(tmp_path / "a"))
    o = _load(tmp_path / "a")
    assert set(o) == {"ray_index", "d_ray", "final", "traj_ray_index", "s_ray", "n_ray"}
    assert all(a.dtype in (np.float32, np.float64) for a in o.values())
    idx = o["ray_index"].astype(np.int64)
    assert len(idx) == 1000 and len(np.unique(idx)) == 1000 and idx.min() >= 0 and idx.max() < R
    assert np.array_equal(o["d_ray"], FakeBatch(R, 1).d_ray()[:, idx])
    assert np.array_equal(o["final"], FakeBatch(R, 1).final()[:, idx])
    t = o["traj_ray_index"].astype(np.int64)
    assert set(t) <= set(idx) and o["s_ray"].shape == (rows, 6, len(t)) and o["n_ray"].shape == (rows, len(t))
    assert np.array_equal(np.rint(o["s_ray"][0, 0]), t) and np.array_equal(np.rint(o["n_ray"][-1]), t)   # ray t, not slot t
    assert sum(a.nbytes for a in o.values()) <= bench.DUMP_BYTES
    # same arguments, same rays: a second run writes the same files
    bench.dump_outputs(FakeBatch(R, rows, perm=perm, n_ray=True), str(tmp_path / "b"))
    for name, a in _load(tmp_path / "b").items():
        assert np.array_equal(a, o[name]), name


def test_dump_keeps_the_records_dtype_and_cuts_a_record_larger_than_the_budget(monkeypatch, tmp_path):
    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)
    R, rows = 50, 20000                                   # one ray's record (480 kB in fp32) alone exceeds the budget
    bench.dump_outputs(FakeBatch(R, rows, dtype=torch.float32), str(tmp_path))
    o = _load(tmp_path)
    assert o["d_ray"].dtype == np.float64 and o["s_ray"].dtype == np.float32
    assert len(o["ray_index"]) == R and o["s_ray"].shape[1:] == (6, 1) and 0 < o["s_ray"].shape[0] < rows
    assert sum(a.nbytes for a in o.values()) <= bench.DUMP_BYTES


def test_dump_of_the_default_workload_fits_64_mb(tmp_path):
    """The bench's default batch: 1 048 576 rays, 3 072 fp64 rows of full record."""
    bench.dump_outputs(FakeBatch(1048576, 3072, lazy=True), str(tmp_path))
    o = _load(tmp_path)
    assert len(o["ray_index"]) == bench.DUMP_RAYS and o["s_ray"].shape[:2] == (3072, 6) and o["s_ray"].shape[2] >= 256
    assert _bytes(tmp_path) <= 64 * 10**6


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_dump_outputs_are_the_same_from_run_to_run(tmp_path):
    """Two runs with different --steps dump the same outputs, bit for bit; at 65 536 rays every ray is in the dump, and the step
    counts of its d_ray add up to the ray-steps of the timed pass that the JSON line reports."""
    lines = []
    for k, steps in ((0, 1), (1, 3)):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--total-rays", "65536", "--steps", str(steps),
                            "--warmup", "1", "--cpu-seconds", "0", "--dump-outputs", str(tmp_path / str(k))],
                           capture_output=True, text=True, timeout=850)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0]))
        assert lines[-1]["steps"] == steps and lines[-1]["parity_check"]["ok"]
    a, b = _load(tmp_path / "0"), _load(tmp_path / "1")
    assert set(a) == {"ray_index", "d_ray", "final", "traj_ray_index", "s_ray"}
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    assert _bytes(tmp_path / "0") <= 64 * 10**6
    assert np.array_equal(a["ray_index"], np.arange(65536)) and a["s_ray"].shape[:2] == (3072, 6)
    for line, d in zip(lines, (a, b)):
        assert int(d["d_ray"][2].sum()) == line["config"]["ray_steps_per_pass_rank0"]
