#!/usr/bin/env python
"""Throughput of the successive-order solver on the headline inputs (bench.py's synthetic snowpacks: 20 layers, IBA
exponential, 32 streams, the 5 AMSR-E channels, 55 deg) at 1024 snowpacks, with n_iteration_max = 8 and then 50.  Prints ONE
JSON line per setting: the resident-input rate in (snowpack, frequency) solves/s, the HIP-event ms of the preparation and
sweep kernels, the rate with H2D + D2H included, the Model.run rate, the share of the FP64 matrix peak the sweep kernel
reaches (2 (2 N)^2 K flop per layer and order run, N = 2 x streams of the layer, K its sublayers) and, for orientation
only, DORT's rate on the same inputs.  No rate is a gate.
   python tools/bench_successive_order.py [n_snowpacks] [steps] [warmup]"""
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

S = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 1
L = 20
from bench import FREQS  # noqa: E402
FREQ = list(FREQS)   # the 5 channels of the headline benchmark
PEAK_FP64_MATRIX = 78.6e12   # MI355X, flop/s
thick, dens, temp, lc = synthetic_snowpacks(seed=0, S=S, L=L)
theta = np.deg2rad([55.0])
batch = PackedBatch([L] * S, thick, dens / 916.7, temp, lc, None, FREQ, theta, emmodel="iba", microstructure="exponential",
                    n_max_stream=32)
ctx = DortContext(0)
N = batch.n_pairs
dort = []
for _ in range(3):
    t0 = time.perf_counter()
    ref = ctx.run(batch)
    dort.append(time.perf_counter() - t0)
packs = [make_snowpack(thick[s], "exponential", density=dens[s], temperature=temp[s], corr_length=lc[s]) for s in range(min(S, 256))]
for n_it in (8, 50):
    ctx.successive_order_upload(batch, n_it, 0.001)
    for _ in range(warmup):
        ctx.successive_order_launch()
    ctx.successive_order_sync()
    prep, sweep, wall = [], [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        ctx.successive_order_launch()
        ctx.successive_order_sync()
        wall.append(time.perf_counter() - t0)
        a, b = ctx.successive_order_kernel_ms()
        prep.append(a)
        sweep.append(b)
    out = ctx.successive_order_download()
    info = ctx.successive_order_launch_info()
    ok = out.status == 0
    n_dir = 4.0 * out.layers[:, :, 4]                                       # 2 N per layer
    flop = float((2.0 * n_dir ** 2 * out.sublayers * np.maximum(out.orders - 1, 0)[:, None])[ok].sum())   # order 0 has no product
    t0 = time.perf_counter()
    ctx.successive_order_run(batch, n_it, 0.001)
    inclusive = time.perf_counter() - t0
    model = make_model("iba", "successive_order", rtsolver_options=dict(n_max_stream=32, n_iteration_max=n_it))
    sensor = sensor_list.passive(FREQ, 55)
    model.run(sensor, packs)
    t0 = time.perf_counter()
    model.run(sensor, packs)
    t_model = time.perf_counter() - t0
    ms = float(np.median(prep) + np.median(sweep))
    gap = np.abs(out.values[ok][:, :, 0, -1] - ref.values[ok][:, :, 0])
    print(json.dumps({
        "metric": "snowpack x frequency successive-order solves/sec (20 layers, 32 streams, n_iteration_max = %d)" % n_it,
        "value": N / ms * 1e3, "unit": "solves/s", "n_gpus": 1, "steps": steps, "warmup": warmup,
        "kernel_ms": {"prep": float(np.median(prep)), "sweep": float(np.median(sweep)), "launch_and_sync_wall_median": float(np.median(wall)) * 1e3},
        "h2d_d2h_inclusive_solves_per_s": N / inclusive, "model_run_solves_per_s": len(packs) * len(FREQ) / t_model,
        "model_run_snowpacks": len(packs), "sweep_flop": flop, "sweep_share_of_fp64_matrix_peak": flop / (float(np.median(sweep)) * 1e-3) / PEAK_FP64_MATRIX,
        "orders_run_mean": float(out.orders[ok].mean()), "sublayers_per_pair_mean": float(out.sublayers[ok].sum(axis=1).mean()),
        "chunks": info["chunks"], "reserved_bytes": info["reserved_bytes"], "failed_solves": int((~ok).sum()),
        "dort_h2d_d2h_inclusive_solves_per_s": N / float(np.median(dort)), "largest_gap_to_dort_K": float(gap.max()) if gap.size else None,
        "dtype": "f64", "data": "synthetic"}))
