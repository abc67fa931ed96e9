"""Times rtmi_kirchhoff_migrate and rtmi_kirchhoff_model on a survey-sized case: vert_heterogeneous closed-form tables (v = 18 +
2 y), 64 sources x 256 receivers drawn from 256 positions at y = -2.4 (16 384 traces, shot-ordered), 512 x 256 nodes over the
box, nt = 2 048 at dt = 0.0005; each kernel without angle bins and with 16.  Medians of --reps calls: the kernel's HIP-event
time (rtmi_kirchhoff_stats.kernel_ms) and the host wall time of the whole call (copies included), against the bytes floor --
every table, trace and image access counted once, at 6 TB/s.  Also the numpy restatement's time on the tests' standard case,
for contrast.  Each case runs in a child process of its own under a time limit, and the first failure ends the run.  Prints
one JSON line per measurement.
--arrivals K times the pair over several arrivals (rtmi_kirchhoff_migrate2 / _model2) on the same case, in one
process with the one-arrival handle it is measured against: the tables replicated into K slots, slot i later by 3 i ms so that
the K^2 pairs of a (trace, node) are distinct and (nearly) all contribute; kmah = slot index.  It prints, for migrate and
model: the one-arrival handle, a create_multi handle of K = 1 without kmah (the same kernel instantiation), and K slots without
and with kmah, each with its time per pair relative to the one-arrival handle.
--antialias NLEV (with --arrivals K, default 1) times the pair anti-aliased by operator slope (rtmi_kirchhoff_create_aa; DESIGN.md
20) on the same case against rtmi_kirchhoff_migrate2 / _model2 on the same inputs, in one process, the two handles called in
turn: pt from the closed-form launch angles, arec = the position spacing (the case is shot gathers), the levels the first NLEV
of 0, 1, 2, 4, 8, 16, 32, 64.  It prints, for migrate and model, the plain kernel, the anti-aliased pair kernel and its filter
(migrate) or sum over the levels (model) apart, their ratio, and the bytes floor with the extra table and the bank.
--lsqr ITERS times least-squares migration on the same case, in one process: the host loop, scipy's lsqr over
as_linear_operator() with atol = btol = 0 and iter_lim = ITERS, and the device loop, Kirchhoff.lsqr, on the same data (the model
of a random reflectivity).  It prints, per iteration: the wall time of each loop, the sum of the two operators' kernel_ms in the
device loop, its vector_ms, and what the device loop's iteration spends above the two kernels.
--hilbert (with --arrivals K, default 2, and --lsqr ITERS, default 3) times the Hilbert transform on the device on
the same case with a handle of K arrivals and kmah, in one process: k_hilbert alone on the [N, nt] traces (the wall time of
Kirchhoff.hilbert_device, which ends with the stream idle: launch, kernel and the wait; median of --reps), rt_bench.hilbert (numpy's
FFT on the host) on the same array for scale, and per iteration the wall time of Kirchhoff.lsqr(hilbert="device") against scipy's
lsqr over as_linear_operator(), whose model and migrate go through the host's FFT.  --lsqr 0 leaves the two loops out.
--filter L (with --arrivals K, default 2, and --lsqr ITERS, default 3) times the trace filter on the device on the
same case with a handle of K arrivals and kmah and L taps (a Ricker convolved with the half-derivative taps), in one process:
k_trace_filter alone in both directions (the wall time of Kirchhoff.filter_device: launch, kernel and the wait; median of --reps)
beside scipy.signal.oaconvolve on the host, and per iteration the wall time of Kirchhoff.lsqr(filtered=True) beside
Kirchhoff.lsqr(hilbert="device") on the same handle and beside the host loop of the same operator -- scipy's lsqr over a
LinearOperator made of model_channels / migrate_channels, rt_bench.hilbert and scipy.signal.oaconvolve -- the two loops
alternating, twice each.  --lsqr 0 leaves the loops out.
--lsqr ITERS --weighted times the weighted loop on the same case and data beside the plain one, in one process, the
two alternating --reps times: row weights, a column scale (1 / sqrt(illumination + 1e-3 max)) and a start model all set.  It
prints, per iteration, the medians and the spread of operator_ms and vector_ms of both loops, the bytes the vector passes of one
iteration move in each, and the kernel time of rtmi_kirchhoff_illumination beside migrate's on the same handle.
Usage: python tools/kirchhoff_timing.py [--reps K] [--case NAME] [--arrivals K] [--antialias NLEV] [--lsqr ITERS] [--hilbert]
                                        [--filter L] [--weighted]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POS_Y = -2.4
CASES = ("migrate", "migrate_bins16", "model", "model_bins16")
LIMIT_S = 240


def tables(pos_x, grid):
    gx0, gdx, nx, gy0, gdy, ny = grid
    X, Y = np.meshgrid(gx0 + np.arange(nx) * gdx, gy0 + np.arange(ny) * gdy)
    T, th = [], []
    for xs in pos_x:
        r2 = (X - xs) ** 2 + (Y - POS_Y) ** 2
        T.append(0.5 * np.arccosh(1.0 + 2.0 * r2 / ((18.0 + 2.0 * POS_Y) * (18.0 + 2.0 * Y))))
        xc = ((X ** 2 - xs ** 2) + (Y + 9) ** 2 - (POS_Y + 9) ** 2) / (2 * (X - xs))
        sg = np.sign(xc - xs)
        th.append(np.arctan2(-sg * (X - xc), sg * (Y + 9)))
    return np.stack(T), np.stack(th)


def run_case(name, reps):
    from raytracing_amd import rt_bench as rb
    P, nt, dt = 256, 2048, 0.0005
    grid = (-2.0, 7.0 / 511, 512, -2.5, 3.5 / 255, 256)
    pos_x = np.linspace(-1.5, 4.5, P) + 1e-3
    T, th = tables(pos_x, grid)
    src = np.arange(0, P, 4)
    isrc = np.repeat(src, P).astype(np.int32)
    irec = np.tile(np.arange(P), len(src)).astype(np.int32)
    N, nn = len(isrc), T[0].size
    nbin = 16 if name.endswith("bins16") else 0
    nb = max(nbin, 1)
    op = rb.Kirchhoff(T, isrc, irec, nt, dt, theta=th if nbin else None, nbin=nbin, dopen=np.pi / 32 if nbin else None)
    rng = np.random.default_rng(1)
    tab = 2 if nbin else 1                                   # T, and theta with bins
    if name.startswith("migrate"):
        x = rng.standard_normal((N, nt))
        call = lambda: op.migrate(x, stats=True)[1]          # noqa: E731
        nbytes = 8 * ((N + len(src)) * nn * tab + N * nt + nb * nn)
    else:
        x = rng.standard_normal((nb,) + T.shape[1:])
        call = lambda: op.model(x, stats=True)[1]            # noqa: E731
        nbytes = 8 * (2 * N * nn * tab + N * nn + N * nt)
    call()                                                   # warm-up: code objects
    ks, ws = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        st = call()
        ws.append((time.perf_counter() - t0) * 1e3)
        ks.append(st["kernel_ms"])
    op.close()
    k = float(np.median(ks))
    print(json.dumps({"what": name, "N": N, "nodes": nn, "nt": nt, "nbin": nbin, "pairs": st["pairs"], "contributing": st["contributing"],
                      "kernel_ms_median": k, "kernel_ms": ks, "wall_ms_median": float(np.median(ws)), "upload_ms": st["upload_ms"],
                      "bytes": nbytes, "floor_ms_at_6TBps": nbytes / 6e12 * 1e3, "pairs_per_s": st["pairs"] / (k * 1e-3),
                      "scale_exp": st["scale_exp"]}), flush=True)


def median_ms(call, reps):
    call()                                                       # warm-up: code objects
    ks = []
    for _ in range(reps):
        st = call()
        ks.append(st["kernel_ms"])
    return float(np.median(ks)), ks, st


def run_arrivals(K, reps):
    from raytracing_amd import rt_bench as rb
    P, nt, dt = 256, 2048, 0.0005
    grid = (-2.0, 7.0 / 511, 512, -2.5, 3.5 / 255, 256)
    pos_x = np.linspace(-1.5, 4.5, P) + 1e-3
    T, _ = tables(pos_x, grid)
    src = np.arange(0, P, 4)
    isrc = np.repeat(src, P).astype(np.int32)
    irec = np.tile(np.arange(P), len(src)).astype(np.int32)
    N, nn = len(isrc), T[0].size
    rng = np.random.default_rng(1)
    d0, d1 = rng.standard_normal((2, N, nt))
    m = rng.standard_normal(T.shape[1:])
    base = {}

    def measure(what, op, karr, kmah):
        for kind in ("migrate", "model"):
            if kind == "migrate":
                call = ((lambda: op.migrate_channels(d0, d1 if kmah else None, stats=True)[1]) if karr
                        else (lambda: op.migrate(d0, stats=True)[1]))
                nbytes = (N + len(src)) * max(karr, 1) * nn * (8 + kmah) + 8 * (N * nt * (1 + kmah) + nn)
            else:
                call = (lambda: op.model_channels(m, stats=True)[1]) if karr else (lambda: op.model(m, stats=True)[1])
                nbytes = 2 * N * max(karr, 1) * nn * (8 + kmah) + 8 * (N * nn + N * nt * (1 + kmah))
            k, ks, st = median_ms(call, reps)
            per_pair = k / st["pairs"]
            base.setdefault(kind, per_pair)                      # the one-arrival handle is measured first
            print(json.dumps({"what": f"{kind}, {what}", "arrivals": karr, "kmah": bool(kmah), "pairs": st["pairs"],
                              "contributing": st["contributing"], "kernel_ms_median": k, "kernel_ms": ks, "bytes": nbytes,
                              "floor_ms_at_6TBps": nbytes / 6e12 * 1e3, "pairs_per_s": st["pairs"] / (k * 1e-3),
                              "ns_per_pair": per_pair * 1e6, "time_per_pair_vs_one_arrival_kernel": per_pair / base[kind]}), flush=True)
        op.close()

    measure("one-arrival handle (rtmi_kirchhoff_create)", rb.Kirchhoff(T, isrc, irec, nt, dt), 0, 0)
    measure("K = 1 without kmah (rtmi_kirchhoff_create_multi)", rb.Kirchhoff(T[:, None], isrc, irec, nt, dt), 1, 0)
    TK = np.stack([T + 0.003 * i for i in range(K)], axis=1)
    if K > 1:
        measure(f"K = {K} without kmah", rb.Kirchhoff(TK, isrc, irec, nt, dt), K, 0)
    km = np.broadcast_to(np.arange(K, dtype=np.float64)[None, :, None, None], TK.shape)
    measure(f"K = {K} with kmah", rb.Kirchhoff(TK, isrc, irec, nt, dt, kmah=km), K, 1)


HW = (0, 1, 2, 4, 8, 16, 32, 64)


def launch_slope(pos_x, grid):
    """pt = -n cos theta0 of the closed form: the launch angle of the arc from (xs, POS_Y) to each node"""
    gx0, gdx, nx, gy0, gdy, ny = grid
    X, Y = np.meshgrid(gx0 + np.arange(nx) * gdx, gy0 + np.arange(ny) * gdy)
    out = []
    for xs in pos_x:
        xc = ((X ** 2 - xs ** 2) + (Y + 9) ** 2 - (POS_Y + 9) ** 2) / (2 * (X - xs))
        sg = np.sign(xc - xs)
        out.append(-np.cos(np.arctan2(-sg * (xs - xc), sg * (POS_Y + 9))) / (18.0 + 2.0 * POS_Y))
    return np.stack(out)


def run_antialias(K, nlev, reps):
    from raytracing_amd import rt_bench as rb
    P, nt, dt = 256, 2048, 0.0005
    grid = (-2.0, 7.0 / 511, 512, -2.5, 3.5 / 255, 256)
    pos_x = np.linspace(-1.5, 4.5, P) + 1e-3
    T, _ = tables(pos_x, grid)
    pt = launch_slope(pos_x, grid)
    src = np.arange(0, P, 4)
    isrc = np.repeat(src, P).astype(np.int32)
    irec = np.tile(np.arange(P), len(src)).astype(np.int32)
    N, nn = len(isrc), T[0].size
    rng = np.random.default_rng(1)
    d0 = rng.standard_normal((N, nt))
    m = rng.standard_normal(T.shape[1:])
    TK = np.stack([T + 0.003 * i for i in range(K)], axis=1)
    PK = np.stack([pt] * K, axis=1)
    aa = dict(hw=HW[:nlev], arec=float(pos_x[1] - pos_x[0]))
    plain = rb.Kirchhoff(TK, isrc, irec, nt, dt)
    anti = rb.Kirchhoff(TK, isrc, irec, nt, dt, pt=PK, antialias=aa)
    sweeps = -(-nt // min(nt, 4096 // nlev))                     # windows of the model kernel: each sweeps the nodes once
    for kind in ("migrate", "model"):
        if kind == "migrate":
            calls = [lambda: plain.migrate_channels(d0, None, stats=True)[1], lambda: anti.migrate_channels(d0, None, stats=True)[1]]
            tab = 8 * (N + len(src)) * K * nn
            nbytes = [tab + 8 * (N * nt + nn), 2 * tab + 8 * (N * nt * (nlev + 2 * (nlev - 1)) + nn)]
        else:
            calls = [lambda: plain.model_channels(m, stats=True)[1], lambda: anti.model_channels(m, stats=True)[1]]
            tab = 8 * 2 * N * K * nn
            nbytes = [tab + 8 * (N * nn + N * nt), sweeps * (2 * tab + 8 * N * nn) + 8 * N * nt * (2 * nlev + 1)]
        for c in calls:
            c()                                                  # warm-up: code objects
        ks, aux = [[], []], []
        for _ in range(reps):                                    # in turn: both see the same state of the device
            for i, c in enumerate(calls):
                st = c()
                ks[i].append(st["kernel_ms"])
                if i:
                    aux.append(st["aux_ms"])
        k0, k1, ax = float(np.median(ks[0])), float(np.median(ks[1])), float(np.median(aux))
        pair = float(np.median(np.array(ks[1]) - np.array(aux)))
        print(json.dumps({"what": f"{kind}, K = {K}, {nlev} levels {list(HW[:nlev])}", "pairs": st["pairs"], "contributing": st["contributing"],
                          "plain_kernel_ms": k0, "aa_total_ms": k1, "aa_pair_kernel_ms": pair,
                          "aa_filter_ms" if kind == "migrate" else "aa_level_sum_ms": ax, "pair_kernel_ratio": pair / k0,
                          "total_ratio": k1 / k0, "model_node_sweeps": sweeps if kind == "model" else None,
                          "plain_bytes": nbytes[0], "aa_bytes": nbytes[1], "plain_floor_ms_at_6TBps": nbytes[0] / 6e12 * 1e3,
                          "aa_floor_ms_at_6TBps": nbytes[1] / 6e12 * 1e3, "plain_kernel_ms_all": ks[0], "aa_total_ms_all": ks[1]}),
              flush=True)
    plain.close(); anti.close()


def run_lsqr(iters):
    from scipy.sparse.linalg import lsqr
    from raytracing_amd import rt_bench as rb
    P, nt, dt = 256, 2048, 0.0005
    grid = (-2.0, 7.0 / 511, 512, -2.5, 3.5 / 255, 256)
    pos_x = np.linspace(-1.5, 4.5, P) + 1e-3
    T, _ = tables(pos_x, grid)
    src = np.arange(0, P, 4)
    isrc = np.repeat(src, P).astype(np.int32)
    irec = np.tile(np.arange(P), len(src)).astype(np.int32)
    op = rb.Kirchhoff(T, isrc, irec, nt, dt)
    d = op.model(np.random.default_rng(1).standard_normal(T.shape[1:]))
    op.lsqr(d, 1)                                                # warm-up: code objects, both operators
    t0 = time.perf_counter()
    dev = op.lsqr(d, iters, stats=True)
    t1 = time.perf_counter()
    host = lsqr(op.as_linear_operator(), d.reshape(-1), atol=0, btol=0, iter_lim=iters)
    t2 = time.perf_counter()
    op.close()
    st = dev["stats"]
    n = dev["itn"]
    # the device loop applies each operator once more than it iterates (the first L^T); scipy's loop does the same
    dev_ms, host_ms = (t1 - t0) * 1e3 / n, (t2 - t1) * 1e3 / host[2]
    print(json.dumps({"what": f"least-squares migration, {iters} iterations", "N": len(isrc), "nodes": T[0].size, "nt": nt,
                      "itn_device": n, "itn_host": int(host[2]), "device_loop_wall_ms_per_iteration": dev_ms,
                      "host_loop_wall_ms_per_iteration": host_ms, "host_over_device": host_ms / dev_ms,
                      "operators_kernel_ms_per_iteration": st["operator_ms"] / n, "vector_ms_per_iteration": st["vector_ms"] / n,
                      "device_loop_above_kernels_ms_per_iteration": dev_ms - st["operator_ms"] / n,
                      "bytes_device": st["bytes_device"], "r1norm_device": dev["r1norm"], "r1norm_host": float(host[3]),
                      "x_max_rel_diff": float(np.max(np.abs(dev["x"].reshape(-1) - host[0])) / np.max(np.abs(host[0])))}), flush=True)


def series(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def run_lsqr_weighted(iters, reps):
    from raytracing_amd import rt_bench as rb
    P, nt, dt = 256, 2048, 0.0005
    grid = (-2.0, 7.0 / 511, 512, -2.5, 3.5 / 255, 256)
    pos_x = np.linspace(-1.5, 4.5, P) + 1e-3
    T, _ = tables(pos_x, grid)
    src = np.arange(0, P, 4)
    isrc = np.repeat(src, P).astype(np.int32)
    irec = np.tile(np.arange(P), len(src)).astype(np.int32)
    N, nn = len(isrc), T[0].size
    op = rb.Kirchhoff(T, isrc, irec, nt, dt)
    rng = np.random.default_rng(1)
    d = op.model(rng.standard_normal(T.shape[1:]))
    x = rng.standard_normal((N, nt))
    ki, kis, sti = median_ms(lambda: op.illumination(stats=True)[1], reps)
    km, kms, stm = median_ms(lambda: op.migrate(x, stats=True)[1], reps)
    print(json.dumps({"what": "rtmi_kirchhoff_illumination beside migrate, kernel event time", "pairs": sti["pairs"],
                      "contributing": sti["contributing"], "migrate_contributing": stm["contributing"], "illumination_ms_median": ki,
                      "migrate_ms_median": km, "illumination_over_migrate": ki / km, "illumination_ms": kis, "migrate_ms": kms}), flush=True)
    opt = dict(row_weight=0.5 + rng.random((N, nt)), col_scale=rb.illumination_scale(op.illumination()), x0=0.1 * rng.standard_normal(T.shape[1:]))
    op.lsqr(d, 1)                                                # warm-up: code objects
    op.lsqr(d, 1, **opt)
    runs = {"plain": [], "weighted": []}
    for _ in range(reps):                                        # alternating: both see the same state of the device
        for name, kw in (("plain", {}), ("weighted", opt)):
            r = op.lsqr(d, iters, stats=True, **kw)
            runs[name].append((r["stats"]["operator_ms"] / r["itn"], r["stats"]["vector_ms"] / r["itn"], r["stats"]["bytes_device"]))
    op.close()
    per, nm = N * nt, nn
    # one iteration's vector passes, every access counted once: axmy (2 reads, 1 write) + sumsq (1) + scale (1, 1) on each side, and
    # x, w (3 reads, 2 writes); weighted: the diagonal read by axmy and by scale, the copy written by scale
    plain_b = 8 * (6 * per + 6 * nm + 5 * nm)
    weighted_b = plain_b + 8 * (3 * per + 3 * nm)
    out = {"what": f"weighted beside plain least-squares migration, {iters} iterations, {reps} alternating runs", "N": N, "nodes": nn, "nt": nt,
           "vector_bytes_per_iteration_plain": plain_b, "vector_bytes_per_iteration_weighted": weighted_b, "byte_ratio": weighted_b / plain_b}
    for name, v in runs.items():
        out[f"{name}_operator_ms_per_iteration"] = series([a[0] for a in v])
        out[f"{name}_vector_ms_per_iteration"] = series([a[1] for a in v])
        out[f"{name}_bytes_device"] = v[0][2]
    out["vector_ms_ratio"] = out["weighted_vector_ms_per_iteration"]["median"] / out["plain_vector_ms_per_iteration"]["median"]
    print(json.dumps(out), flush=True)


def run_hilbert(K, reps, iters):
    import torch
    from scipy.sparse.linalg import lsqr
    from raytracing_amd import rt_bench as rb
    P, nt, dt = 256, 2048, 0.0005
    grid = (-2.0, 7.0 / 511, 512, -2.5, 3.5 / 255, 256)
    pos_x = np.linspace(-1.5, 4.5, P) + 1e-3
    T, _ = tables(pos_x, grid)
    src = np.arange(0, P, 4)
    isrc = np.repeat(src, P).astype(np.int32)
    irec = np.tile(np.arange(P), len(src)).astype(np.int32)
    N = len(isrc)
    TK = np.stack([T + 0.003 * i for i in range(K)], axis=1)
    km = np.broadcast_to(np.arange(K, dtype=np.float64)[None, :, None, None], TK.shape)
    op = rb.Kirchhoff(TK, isrc, irec, nt, dt, kmah=km)
    x = np.random.default_rng(1).standard_normal((N, nt))
    tx = torch.from_numpy(x).to("cuda")
    op.hilbert_device(tx)                                        # warm-up: code object, the taps
    ws = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ty = op.hilbert_device(tx)
        ws.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    hf = rb.hilbert(x)
    fft_ms = (time.perf_counter() - t0) * 1e3
    diff = float(np.max(np.abs(ty.cpu().numpy() - hf)) / np.max(np.abs(hf)))
    taps = nt // 4 if nt % 2 == 0 else (nt - 1) // 2
    # the fp64 floor: 3 operations per output and tap, 4 cycles per wave instruction, 1024 SIMDs at 2.4 GHz
    floor_ms = N * nt * taps * 3 / 64 * 4 / 1024 / 2.4e9 * 1e3
    k = float(np.median(ws))
    print(json.dumps({"what": "k_hilbert alone (launch, kernel, wait)", "N": N, "nt": nt, "taps": taps, "wall_ms_median": k, "wall_ms": ws,
                      "fp64_issue_floor_ms": floor_ms, "wall_over_fp64_floor": k / floor_ms, "numpy_fft_on_the_host_ms": fft_ms,
                      "max_diff_from_fft_over_max": diff}), flush=True)
    if iters > 0:
        d = op.model(np.random.default_rng(1).standard_normal(T.shape[1:]))
        op.lsqr(d, 1, hilbert="device")                          # warm-up: code objects, both operators
        t0 = time.perf_counter()
        dev = op.lsqr(d, iters, stats=True, hilbert="device")
        t1 = time.perf_counter()
        host = lsqr(op.as_linear_operator(), d.reshape(-1), atol=0, btol=0, iter_lim=iters)
        t2 = time.perf_counter()
        st, n = dev["stats"], dev["itn"]
        dev_ms, host_ms = (t1 - t0) * 1e3 / n, (t2 - t1) * 1e3 / host[2]
        print(json.dumps({"what": f"least-squares migration of the full trace, K = {K} with kmah, {iters} iterations", "N": N,
                          "nodes": T[0].size, "nt": nt, "itn_device": n, "itn_host": int(host[2]),
                          "device_loop_wall_ms_per_iteration": dev_ms, "host_loop_wall_ms_per_iteration": host_ms,
                          "host_over_device": host_ms / dev_ms, "operators_kernel_ms_per_iteration": st["operator_ms"] / n,
                          "vector_ms_per_iteration": st["vector_ms"] / n, "bytes_device": st["bytes_device"],
                          "r1norm_device": dev["r1norm"], "r1norm_host": float(host[3]),
                          "x_max_rel_diff": float(np.max(np.abs(dev["x"].reshape(-1) - host[0])) / np.max(np.abs(host[0])))}), flush=True)
    op.close()


def run_filter(L, K, reps, iters):
    import torch
    from scipy.signal import oaconvolve
    from scipy.sparse.linalg import LinearOperator, lsqr
    from raytracing_amd import rt_bench as rb
    P, nt, dt = 256, 2048, 0.0005
    grid = (-2.0, 7.0 / 511, 512, -2.5, 3.5 / 255, 256)
    pos_x = np.linspace(-1.5, 4.5, P) + 1e-3
    T, _ = tables(pos_x, grid)
    src = np.arange(0, P, 4)
    isrc = np.repeat(src, P).astype(np.int32)
    irec = np.tile(np.arange(P), len(src)).astype(np.int32)
    N = len(isrc)
    TK = np.stack([T + 0.003 * i for i in range(K)], axis=1)
    km = np.broadcast_to(np.arange(K, dtype=np.float64)[None, :, None, None], TK.shape)
    op = rb.Kirchhoff(TK, isrc, irec, nt, dt, kmah=km)
    # a zero-phase Ricker of 2 M + 1 taps convolved with the half-derivative: L taps, the origin at the Ricker's centre
    M = min(32, (L - 1) // 2)
    u = (np.pi * 60.0 * (np.arange(2 * M + 1) - M) * dt) ** 2
    f = np.convolve((1.0 - 2.0 * u) * np.exp(-u), rb.half_derivative_taps(L - 2 * M, dt))
    assert f.size == L
    op.set_filter(f, origin=M)

    def host_F(b, transpose=False):
        g = f[::-1] if transpose else f
        o = L - 1 - M if transpose else M
        return oaconvolve(b, g[None, :], axes=-1)[:, o:o + nt]

    x = np.random.default_rng(1).standard_normal((N, nt))
    tx = torch.from_numpy(x).to("cuda")
    # the fp64 floor: 2 operations per output and tap, 4 cycles per wave instruction, 1024 SIMDs at 2.4 GHz
    floor_ms = N * nt * L * 2 / 64 * 4 / 1024 / 2.4e9 * 1e3
    for tr in (False, True):
        op.filter_device(tx, transpose=tr)                       # warm-up: code object
        ws = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ty = op.filter_device(tx, transpose=tr)
            ws.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        hf = host_F(x, tr)
        host_ms = (time.perf_counter() - t0) * 1e3
        k = float(np.median(ws))
        print(json.dumps({"what": f"k_trace_filter<{'true' if tr else 'false'}> alone (launch, kernel, wait)", "N": N, "nt": nt, "taps": L,
                          "origin": M, "wall_ms_median": k, "wall_ms": ws, "fp64_issue_floor_ms": floor_ms,
                          "wall_over_fp64_floor": k / floor_ms, "scipy_oaconvolve_on_the_host_ms": host_ms,
                          "max_diff_from_host_over_max": float(np.max(np.abs(ty.cpu().numpy() - hf)) / np.max(np.abs(hf)))}), flush=True)
    if iters > 0:
        shape = T.shape[1:]

        def matvec(m):
            c0, c1 = op.model_channels(m.reshape(shape))
            return host_F(c0 + rb.hilbert(c1)).reshape(-1)

        def rmatvec(u):
            ft = host_F(u.reshape(N, nt), transpose=True)
            return op.migrate_channels(ft, -rb.hilbert(ft)).reshape(-1)
        host_op = LinearOperator(op.shape, matvec=matvec, rmatvec=rmatvec, dtype=np.float64)
        d = np.ascontiguousarray(matvec(np.random.default_rng(1).standard_normal(shape)).reshape(N, nt))
        op.lsqr(d, 1, hilbert="device", filtered=True)           # warm-up: code objects, all operators
        op.lsqr(d, 1, hilbert="device")
        for run in (1, 2):
            t0 = time.perf_counter()
            dev = op.lsqr(d, iters, stats=True, hilbert="device", filtered=True)
            t1 = time.perf_counter()
            host = lsqr(host_op, d.reshape(-1), atol=0, btol=0, iter_lim=iters)
            t2 = time.perf_counter()
            plain = op.lsqr(d, iters, stats=True, hilbert="device")
            t3 = time.perf_counter()
            st, n = dev["stats"], dev["itn"]
            dev_ms, host_ms, plain_ms = (t1 - t0) * 1e3 / n, (t2 - t1) * 1e3 / host[2], (t3 - t2) * 1e3 / plain["itn"]
            print(json.dumps({"what": f"least-squares migration with the filter inside, K = {K} with kmah, L = {L}, {iters} iterations, "
                                      f"run {run}", "N": N, "nodes": T[0].size, "nt": nt, "itn_device": n, "itn_host": int(host[2]),
                              "filtered_device_loop_wall_ms_per_iteration": dev_ms,
                              "unfiltered_device_loop_wall_ms_per_iteration": plain_ms, "filtered_over_unfiltered": dev_ms / plain_ms,
                              "host_loop_wall_ms_per_iteration": host_ms, "host_over_device": host_ms / dev_ms,
                              "operators_kernel_ms_per_iteration": st["operator_ms"] / n,
                              "unfiltered_operators_kernel_ms_per_iteration": plain["stats"]["operator_ms"] / plain["itn"],
                              "library_total_ms_per_iteration": st["total_ms"] / n,
                              "unfiltered_library_total_ms_per_iteration": plain["stats"]["total_ms"] / plain["itn"],
                              "vector_ms_per_iteration": st["vector_ms"] / n, "bytes_device": st["bytes_device"],
                              "r1norm_device": dev["r1norm"], "r1norm_host": float(host[3]),
                              "x_max_rel_diff": float(np.max(np.abs(dev["x"].reshape(-1) - host[0])) / np.max(np.abs(host[0])))}),
                  flush=True)
    op.close()


def restatement():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import kirchhoff_ref as K
    isrc, irec = K.geometry()
    T = K.closed_T()
    d = K.scatterer_data(isrc, irec)
    t0 = time.perf_counter()
    _, cnt = K.migrate(T, isrc, irec, d, K.DT)
    t = time.perf_counter() - t0
    print(json.dumps({"what": "numpy restatement, migrate, standard case", "pairs": len(isrc) * T[0].size, "contributing": cnt,
                      "seconds": t, "pairs_per_s": len(isrc) * T[0].size / t}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", choices=CASES + ("restatement",))
    ap.add_argument("--arrivals", type=int, choices=(1, 2, 3, 4))
    ap.add_argument("--antialias", type=int, choices=range(1, 9), metavar="NLEV")
    ap.add_argument("--lsqr", type=int, metavar="ITERS")
    ap.add_argument("--hilbert", action="store_true")
    ap.add_argument("--filter", type=int, metavar="L")
    ap.add_argument("--weighted", action="store_true")
    a = ap.parse_args()
    if a.filter:
        if not 3 <= a.filter <= 2048:
            ap.error("--filter L: 3 <= L <= 2048")
        run_filter(a.filter, a.arrivals or 2, a.reps, 3 if a.lsqr is None else a.lsqr)
    elif a.hilbert:
        run_hilbert(a.arrivals or 2, a.reps, 3 if a.lsqr is None else a.lsqr)
    elif a.lsqr and a.weighted:
        run_lsqr_weighted(a.lsqr, a.reps)
    elif a.lsqr:
        run_lsqr(a.lsqr)
    elif a.antialias:
        run_antialias(a.arrivals or 1, a.antialias, a.reps)
    elif a.arrivals:
        run_arrivals(a.arrivals, a.reps)
    elif a.case == "restatement":
        restatement()
    elif a.case:
        run_case(a.case, a.reps)
    else:
        for c in CASES + ("restatement",):
            rc = subprocess.call(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--case", c,
                                  "--reps", str(a.reps)])
            if rc != 0:
                sys.exit(f"kirchhoff_timing: case {c} ended with status {rc}; stopping")
