"""Per-ray parity measures for whole fans (imported by tests; not collected: no test_ prefix).

Arrays are laid out [.., quantity, ray] like bench.parity_relerr's: a final state [9, R], d_ray [3, R] or [2, R], recorded
rows [rows, 6, R].  They may be torch tensors on any device or numpy arrays; the work stays where the data is, so a 30 GB
record is compared on the GPU in chunks of rays and only per-ray results come back.

Each ray's error is the larger of bench.py's two measures, restricted to that ray:
  * parity_relerr: |a - b| over ONE scale per quantity group (QUANTITY_GROUPS), the largest |b| of that group over the WHOLE
    batch -- every row and every ray, not the chunk's -- and for the final state's grad-n group at least the index's scale;
  * parity_relerr_elementwise: |a - b| / max(|b|, 1).
Division is monotone, so the maximum of the per-ray errors is the batch-wide value bench.py computes, to the last bit.  A NaN
on either side (or an infinity) makes that ray's error +inf: offenders are ~(err <= tol), which a NaN cannot slip through.
"""
import math

import numpy as np
import torch

from bench import QUANTITY_GROUPS

CHUNK = 1 << 16
GROUP_NAMES = {9: ("x y", "theta", "n", "dn/dx dn/dy", "p_x p_y", "T"), 6: ("x y", "p_x p_y", "T", "theta"),
               3: ("dist_real dist_sim", "last row"), 2: ("dist_real dist_sim",)}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a


def _ranges(R, chunk):
    chunk = int(chunk) if chunk else R
    return [(r0, min(r0 + chunk, R)) for r0 in range(0, max(R, 1), chunk)] if R else []


def _groups(Q):
    # every group of QUANTITY_GROUPS is a run of consecutive quantities: (first, count)
    return [(g[0], len(g)) for g in QUANTITY_GROUPS[Q]]


def group_scales(b, chunk=CHUNK):
    """First pass: the scale of every quantity group over the whole of b (NaNs ignored here; they fail their own ray)."""
    b = _t(b)
    Q, R = b.shape[-2], b.shape[-1]
    lead = tuple(range(b.dim() - 2))
    best = torch.zeros(Q, dtype=torch.float64, device=b.device)
    for r0, r1 in _ranges(R, chunk):
        m = torch.nan_to_num(b[..., r0:r1].to(torch.float64).abs(), nan=0.0).amax(dim=lead + (b.dim() - 1,))
        best = torch.maximum(best, m)
    best = best.cpu().numpy()
    scales = []
    for q0, n in _groups(Q):
        s = float(best[q0:q0 + n].max())
        if Q == 9 and q0 == 4:
            s = max(s, float(best[3]))          # grad n: at least the index's own scale (bench.parity_relerr)
        scales.append(s)
    return scales


def per_ray_error(a, b, chunk=CHUNK, scales=None):
    """(err [R] float64, group [R] int64) on b's device: each ray's larger error under the two measures, and the index into
    QUANTITY_GROUPS[Q] of the group it comes from.  NaN -> +inf."""
    a, b = _t(a), _t(b)
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    Q, R = b.shape[-2], b.shape[-1]
    if scales is None:
        scales = group_scales(b, chunk)
    red = tuple(range(b.dim() - 2))
    err = torch.empty(R, dtype=torch.float64, device=b.device)
    grp = torch.empty(R, dtype=torch.int64, device=b.device)
    for r0, r1 in _ranges(R, chunk):
        bc = b[..., r0:r1].to(torch.float64)
        d = (a[..., r0:r1].to(torch.float64) - bc).abs_()
        el = d / bc.abs().clamp_min_(1.0)           # NaN stays NaN through abs and clamp_min
        per = []
        for (q0, n), s in zip(_groups(Q), scales):
            dg = d.narrow(-2, q0, n).amax(dim=red + (-2,))
            rel = dg / s if s > 0.0 else torch.full_like(dg, math.inf)
            rel = torch.where(dg == 0, torch.zeros_like(rel), rel)       # 0/0 where the group is zero; NaN stays NaN
            eg = el.narrow(-2, q0, n).amax(dim=red + (-2,))
            per.append(torch.maximum(rel, eg))
        per = torch.nan_to_num(torch.stack(per), nan=math.inf)
        err[r0:r1], grp[r0:r1] = per.max(dim=0)
        del bc, d, el, per
    return err, grp


def worst(err, k=5):
    """Indices of the k largest errors, largest first (an +inf -- a NaN -- first of all)."""
    err = _t(err)
    k = min(int(k), err.numel())
    return torch.topk(err, k).indices.cpu().numpy() if k else np.zeros(0, np.int64)


def offenders(err, tol):
    """Indices of the rays NOT within tol: ~(err <= tol), so a NaN (mapped to +inf, or left as NaN) is one."""
    err = _t(err)
    return torch.nonzero(~(err <= tol)).flatten().cpu().numpy()


def describe(err, grp, Q, theta, rays):
    """One line per ray: index, launch angle, quantity group and error -- for failure messages and -s output."""
    err, grp = _t(err), _t(grp)
    names = GROUP_NAMES[Q]
    out = []
    for i in rays:
        i = int(i)
        out.append(f"ray {i} (theta {float(theta[i]):.15g} rad = {math.degrees(float(theta[i])):.10g} deg): "
                   f"{names[int(grp[i])]} {float(err[i]):.3e}")
    return "; ".join(out)


class Compared:
    """err/grp of one comparison plus what a message needs."""

    def __init__(self, a, b, theta, chunk=CHUNK):
        self.err, self.grp = per_ray_error(a, b, chunk)
        self.Q, self.theta = _t(b).shape[-2], theta

    @property
    def max(self):
        return float(self.err.max()) if self.err.numel() else 0.0

    def beyond(self, tol):
        return offenders(self.err, tol)

    def report(self, k=3, rays=None):
        return describe(self.err, self.grp, self.Q, self.theta, worst(self.err, k) if rays is None else rays[:k])


def fingerprint(rows, chunk=CHUNK):
    """[Q, R] int64: per ray and quantity, the wrap-around sum of the rows' bits as integers -- equal for equal bits (a cheap
    exact comparison of two runs' records without keeping a copy of either)."""
    rows = _t(rows)
    bits = rows.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[rows.element_size()])     # same element size: any strides
    Q, R = rows.shape[-2], rows.shape[-1]
    out = torch.empty((Q, R), dtype=torch.int64, device=rows.device)
    red = tuple(range(rows.dim() - 2))
    for r0, r1 in _ranges(R, chunk):
        c = bits[..., r0:r1]
        out[:, r0:r1] = c.sum(dim=red, dtype=torch.int64) if red else c.to(torch.int64)
    return out
