#!/usr/bin/env python
"""Throughput of the iterative second-order solver: 3-layer IBA exponential snowpacks (seed 4) at 13 GHz, 3 incidence
angles, the solver's defaults (n_max_stream=32, m_max=5), Flat substrate, at 2 048 snowpacks.  Prints ONE JSON line per
setting of compute_scattering_interlayer (off, on): the resident-input rate in (snowpack, frequency) solves/s, the HIP-event
ms of the first-order and of the order-2 kernels, the rate with H2D + D2H included, the Model.run rate and, for scale, the
rate of the NumPy restatement on the host.  No rate is a gate.
   python tools/bench_second_order.py [n_snowpacks] [steps] [warmup]"""
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
from smrt_amd._native import DortContext, PackedBatch, PackedSecondOrderExtras  # noqa: E402
from smrt_amd.inputs.make_medium import make_snowpack, make_soil  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 2
L, FREQ, NMAX, MMAX = 3, 13e9, 32, 5
theta_deg = np.array([20.0, 35.0, 50.0])
thick, dens, temp, lc = synthetic_snowpacks(seed=4, S=S, L=L, thick_range=(0.1, 0.5), last=0.6)
batch = PackedBatch([L] * S, thick, dens / 916.7, temp, lc, None, [FREQ], np.deg2rad(theta_deg), emmodel="iba",
                    microstructure="exponential", mode="A", n_max_stream=NMAX, m_max=MMAX, substrate=("flat", 8.0, 1.0, [268.0] * S))
ctx = DortContext(0)
for interlayer in (False, True):
    extras = PackedSecondOrderExtras(batch, interlayer)
    ctx.second_order_upload(batch, extras)
    for _ in range(warmup):
        ctx.second_order_launch()
    ctx.second_order_sync()
    ms_a, ms_b, wall = [], [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        ctx.second_order_launch()
        ctx.second_order_sync()
        wall.append((time.perf_counter() - t0) * 1e3)
        a, b = ctx.second_order_kernel_ms()
        ms_a.append(a)
        ms_b.append(b)
    out = ctx.second_order_download()
    ms = float(np.median(ms_a) + np.median(ms_b))
    inclusive = []
    for _ in range(max(3, steps // 4)):
        t0 = time.perf_counter()
        ctx.second_order_run(batch, extras)
        inclusive.append(time.perf_counter() - t0)
    n_model = min(S, 1024)
    soil = make_soil("flat", complex(8.0, 1.0), 268.0)
    packs = [make_snowpack(thick[s], "exponential", density=dens[s], temperature=temp[s], corr_length=lc[s], substrate=soil) for s in range(n_model)]
    model = make_model("iba", "iterative_second_order", rtsolver_options=dict(compute_scattering_interlayer=interlayer))
    sensor = sensor_list.active(FREQ, theta_deg)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = model.run(sensor, packs)
        t0 = time.perf_counter()
        res = model.run(sensor, packs)
        t_model = time.perf_counter() - t0
    from oracle import dort_oracle as O  # noqa: E402
    from second_order_restatement import second_order  # noqa: E402
    n_host = 2
    t0 = time.perf_counter()
    worst = 0.0
    for s in range(n_host):
        layers = O.make_layers("iba", FREQ, dict(thickness=thick[s], density=dens[s], temperature=temp[s], microstructure="exponential",
                                                 corr_length=lc[s]))
        ref, _ = second_order(layers, thick[s], FREQ, theta_deg, None, ("flat", complex(8.0, 1.0)), NMAX, MMAX, interlayer)
        worst = max(worst, np.abs(out.values[s] - ref).max() / max(ref.sum(axis=0)[:, 0, 0].max(), ref.sum(axis=0)[:, 1, 1].max()))
    t_host = (time.perf_counter() - t0) / n_host
    print(json.dumps({
        "metric": "snowpack x frequency second-order backscatter solves/sec (3 layers, 3 incidence angles, 32 streams, m_max 5)",
        "compute_scattering_interlayer": interlayer,
        "value": S / ms * 1e3, "unit": "solves/s", "n_gpus": 1, "steps": steps, "warmup": warmup,
        "kernel_ms": {"first_order": float(np.median(ms_a)), "order2": float(np.median(ms_b)), "order2_min": float(np.min(ms_b)),
                      "launch_and_sync_wall_median": float(np.median(wall))},
        "h2d_d2h_inclusive_solves_per_s": S / float(np.median(inclusive)),
        "model_run_solves_per_s": n_model / t_model, "model_run_snowpacks": n_model,
        "numpy_restatement_solves_per_s": 1.0 / t_host, "worst_error_vs_restatement": worst,
        "failed_solves": int((out.status != 0).sum()), "dtype": "f64", "data": "synthetic",
        "config": "IBA exponential, 13 GHz, 20 / 35 / 50 deg, 3 layers, Flat substrate, %d snowpacks" % S}))
