#!/usr/bin/env python
"""Throughput of the iterative first-order solver on the BASELINE configs[3] inputs (seed 4, 30 layers, IBA exponential,
Sentinel-1 5.405 GHz, theta_inc 20..45 deg) at 16 384 snowpacks.  Prints ONE JSON line: the resident-input rate in
(snowpack, frequency) solves/s and in (solve, angle) items/s, the HIP-event ms of the two kernels, the rate with H2D + D2H
included, the Model.run rate and, for scale, the rate of the NumPy restatement on the host.  No rate is a gate.
   python tools/bench_first_order.py [n_snowpacks] [steps] [warmup]"""
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench import synthetic_snowpacks  # noqa: E402
from smrt_amd import make_model, sensor_list  # noqa: E402
from smrt_amd._native import DortContext, PackedBatch  # noqa: E402
from smrt_amd.inputs.make_medium import make_snowpack  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 3
L = 30
theta_deg = np.arange(20.0, 46.0, 5.0)
thick, dens, temp, lc = synthetic_snowpacks(seed=4, S=S, L=L, thick_range=(0.02, 0.10), last=1000.0)
batch = PackedBatch([L] * S, thick, dens / 916.7, temp, lc, None, [5.405e9], np.deg2rad(theta_deg), emmodel="iba",
                    microstructure="exponential", mode="A")
ctx = DortContext(0)
ctx.first_order_upload(batch)
for _ in range(warmup):
    ctx.first_order_launch()
ctx.first_order_sync()
ms_a, ms_b, wall = [], [], []
for _ in range(steps):   # one launch per sample: HIP events per kernel, wall clock around launch + sync
    t0 = time.perf_counter()
    ctx.first_order_launch()
    ctx.first_order_sync()
    wall.append((time.perf_counter() - t0) * 1e3)
    a, b = ctx.first_order_kernel_ms()
    ms_a.append(a)
    ms_b.append(b)
out = ctx.first_order_download()
ms = float(np.median(ms_a) + np.median(ms_b))
inclusive = []
for _ in range(max(3, steps // 4)):
    t0 = time.perf_counter()
    ctx.first_order_run(batch)
    inclusive.append(time.perf_counter() - t0)
n_model = min(S, 2048)   # Model.run builds Python snowpack objects: a slice keeps the benchmark short
packs = [make_snowpack(thick[s], "exponential", density=dens[s], temperature=temp[s], corr_length=lc[s]) for s in range(n_model)]
model = make_model("iba", "iterative_first_order")
sensor = sensor_list.active(5.405e9, theta_deg)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    res = model.run(sensor, packs)
    t0 = time.perf_counter()
    res = model.run(sensor, packs)
    t_model = time.perf_counter() - t0
assert np.array_equal(res.data.values, out.values[:n_model].sum(axis=1))
from first_order_restatement import first_order  # noqa: E402
from oracle import dort_oracle as O  # noqa: E402
n_host = 8
t0 = time.perf_counter()
worst = 0.0
for s in range(n_host):
    layers = O.make_layers("iba", 5.405e9, dict(thickness=thick[s], density=dens[s], temperature=temp[s], microstructure="exponential",
                                                corr_length=lc[s]))
    ref, _ = first_order(layers, thick[s], 5.405e9, theta_deg)
    worst = max(worst, np.abs(out.values[s] - ref).max() / ref.sum(axis=0)[:, 0, 0].max())
t_host = (time.perf_counter() - t0) / n_host
print(json.dumps({
    "metric": "snowpack x frequency first-order backscatter solves/sec (30 layers, 6 incidence angles)",
    "value": S / ms * 1e3, "unit": "solves/s", "items_per_s": S * len(theta_deg) / ms * 1e3, "n_gpus": 1, "steps": steps, "warmup": warmup,
    "kernel_ms": {"layers": float(np.median(ms_a)), "angles": float(np.median(ms_b)), "layers_min": float(np.min(ms_a)),
                  "angles_min": float(np.min(ms_b)), "launch_and_sync_wall_median": float(np.median(wall))},
    "h2d_d2h_inclusive_solves_per_s": S / float(np.median(inclusive)),
    "model_run_solves_per_s": n_model / t_model, "model_run_snowpacks": n_model,
    "numpy_restatement_solves_per_s": 1.0 / t_host, "worst_error_vs_restatement": worst,
    "failed_solves": int((out.status != 0).sum()), "dtype": "f64", "data": "synthetic",
    "config": "BASELINE configs[3] inputs: IBA exponential, Sentinel-1 5.405 GHz, 20..45 deg, 30 layers, %d snowpacks, no substrate" % S}))
