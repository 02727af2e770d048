#!/usr/bin/env python
"""Throughput of the successive-order backscatter solver on synthetic snowpacks (bench.py's generator: 30 layers, IBA
exponential, 32 streams, 13 GHz, 8 orders) at 16 384 snowpacks, with 1 incidence angle and then 6.  Prints ONE JSON line per
setting: the resident-input rate in (snowpack, frequency) solves/s, the HIP-event ms of the preparation, sweep and combine
kernels, the rate with H2D + D2H included, the Model.run rate, the share of the FP64 matrix peak the sweep kernel reaches
(2 (6 n)^2 K C flop per layer, mode pass and order after the first, n the streams of the layer, K its sublayers, C the
columns) and, for orientation only, the time of active DORT and of iterative_first_order on the same inputs.  No rate is a gate.
   python tools/bench_successive_order_active.py [n_snowpacks] [steps] [warmup]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import synthetic_snowpacks  # noqa: E402
from smrt_amd import make_model, sensor_list  # noqa: E402
from smrt_amd._native import DortContext, PackedBatch  # noqa: E402
from smrt_amd.inputs.make_medium import make_snowpack  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 2
L, N_IT, FREQ = 30, 8, [13e9]
PEAK_FP64_MATRIX = 78.6e12   # MI355X, flop/s
thick, dens, temp, lc = synthetic_snowpacks(seed=0, S=S, L=L)
ctx = DortContext(0)
packs = [make_snowpack(thick[s], "exponential", density=dens[s], temperature=temp[s], corr_length=lc[s]) for s in range(min(S, 256))]
for angles in ([40.0], [20.0, 28.0, 36.0, 44.0, 52.0, 60.0]):
    theta = np.deg2rad(angles)
    batch = PackedBatch([L] * S, thick, dens / 916.7, temp, lc, None, FREQ, theta, emmodel="iba", microstructure="exponential",
                        n_max_stream=32, mode="A", m_max=2)
    N = batch.n_pairs
    ctx.run(batch)                                                          # warm: the first call allocates
    dort = []
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.run(batch)
        dort.append(time.perf_counter() - t0)
    t_dort = float(np.median(dort))
    ctx.so_active_upload(batch, theta, N_IT, 0.001)
    for _ in range(warmup):
        ctx.so_active_launch()
    ctx.so_active_sync()
    ms, wall = [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        ctx.so_active_launch()
        ctx.so_active_sync()
        wall.append(time.perf_counter() - t0)
        ms.append(ctx.so_active_kernel_ms())
    out = ctx.so_active_download()
    info = ctx.so_active_launch_info()
    ok = out.status == 0
    prep, sweep, combine = (float(v) for v in np.median(np.array(ms), axis=0))
    columns = 2.0 * min(2 * len(angles), 32)                                # an upper bound: bracketing streams may coincide
    n_dir = 6.0 * out.layers[:, :, 4]
    products = np.maximum(out.orders[:, 1:] - 1, 0).sum(axis=1)            # mode passes only; order 0 has no product
    flop = float((2.0 * n_dir ** 2 * out.sublayers * columns * products[:, None])[ok].sum())
    t0 = time.perf_counter()
    ctx.so_active_run(batch, theta, N_IT, 0.001)
    inclusive = time.perf_counter() - t0
    sensor = sensor_list.active(FREQ[0], angles)
    rates = {}
    for name, options in (("successive_order_backscatter", dict(n_max_stream=32, n_iteration_max=N_IT)), ("iterative_first_order", {})):
        model = make_model("iba", name, rtsolver_options=options)
        model.run(sensor, packs)
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            model.run(sensor, packs)
            runs.append(time.perf_counter() - t0)
        rates[name] = len(packs) / float(np.median(runs))
    print(json.dumps({
        "metric": "snowpack x frequency successive-order backscatter solves/sec (30 layers, 32 streams, %d angle(s), 8 orders)" % len(angles),
        "value": N / (prep + sweep + combine) * 1e3, "unit": "solves/s", "n_gpus": 1, "steps": steps, "warmup": warmup,
        "kernel_ms": {"prep": prep, "sweep": sweep, "combine": combine, "launch_and_sync_wall_median": float(np.median(wall)) * 1e3},
        "h2d_d2h_inclusive_solves_per_s": N / inclusive, "model_run_solves_per_s": rates["successive_order_backscatter"],
        "model_run_snowpacks": len(packs), "sweep_flop_upper_bound": flop,
        "sweep_share_of_fp64_matrix_peak": flop / (sweep * 1e-3) / PEAK_FP64_MATRIX,
        "orders_run_mean": float(out.orders[ok].mean()), "sublayers_per_pair_mean": float(out.sublayers[ok].sum(axis=1).mean()),
        "chunks": info["chunks"], "reserved_bytes": info["reserved_bytes"], "failed_solves": int((~ok).sum()),
        "dort_active_h2d_d2h_inclusive_solves_per_s": N / t_dort, "iterative_first_order_model_run_solves_per_s": rates["iterative_first_order"],
        "samples": {"kernel_ms": "median of %d launches after %d warm-up" % (steps, warmup), "h2d_d2h_inclusive": "one warm call",
                    "model_run": "median of 3 warm calls on %d snowpacks" % len(packs), "dort_active": "median of 3 warm calls"},
        "dtype": "f64", "data": "synthetic"}))
