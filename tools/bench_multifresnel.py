#!/usr/bin/env python
"""Throughput of the multi-Fresnel thermal emission solver on firn-like profiles (layers of 5 cm, density rising with depth,
1.4 GHz, 8 angles, non-scattering layers): by default 16 384 pairs at 300 layers and 256 pairs at 4000 layers.  Prints ONE JSON
line per batch: the resident-input rate in (snowpack, frequency) solves/s -- median and spread of the HIP-event times of the
two kernels over `steps` launches after `warmup` --, the rate with H2D + D2H included, the Model.run rate and, as the
comparison a user has today, the existing dort solver on the same non-scattering layers on the device at the fewest streams
that resolve the 8 angles (n_max_stream = 16), on `dort_pairs` of the pairs.  No rate is a gate.
   python tools/bench_multifresnel.py [steps] [warmup] [dort_pairs] [pairs:layers ...]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from smrt_amd import make_model, sensor_list  # noqa: E402
from smrt_amd._native import DortContext, PackedBatch  # noqa: E402
from smrt_amd.inputs.make_medium import make_snowpack  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 2
dort_pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 256
shapes = [tuple(int(v) for v in a.split(":")) for a in sys.argv[4:]] or [(16384, 300), (256, 4000)]
FREQUENCY = 1.4e9
THETA = [0.0, 10.0, 20.0, 30.0, 40.0, 50.0, 55.0, 60.0]
DORT_STREAMS = 16
DORT_MAX_LAYERS = 300


def profiles(S, L, seed=0):
    rng = np.random.RandomState(seed)
    z = (np.arange(L) + 0.5) * 0.05
    density = 350.0 + 450.0 * (1.0 - np.exp(-z / 60.0)) + rng.uniform(-30.0, 30.0, (S, L))
    temperature = 245.0 + 12.0 * np.exp(-z / 3.0) * np.cos(z / 3.0) + rng.uniform(-0.2, 0.2, (S, L))
    return np.full((S, L), 0.05), density, temperature


def spread(values):
    v = np.asarray(values, float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


ctx = DortContext(0)
mu = np.cos(np.deg2rad(THETA))
for S, L in shapes:
    thick, dens, temp = profiles(S, L)
    batch = PackedBatch([L] * S, thick, dens / 916.7, temp, np.full((S, L), 1e-4), None, [FREQUENCY], np.deg2rad(THETA),
                        emmodel="nonscattering", microstructure="exponential", n_max_stream=DORT_STREAMS)
    ctx.multifresnel_upload(batch, mu, 10)
    for _ in range(warmup):
        ctx.multifresnel_launch()
    ctx.multifresnel_sync()
    layers_ms, chain_ms, wall = [], [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        ctx.multifresnel_launch()
        ctx.multifresnel_sync()
        wall.append((time.perf_counter() - t0) * 1e3)
        a, b = ctx.multifresnel_kernel_ms()
        layers_ms.append(a)
        chain_ms.append(b)
    out = ctx.multifresnel_download()
    inclusive = []
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.multifresnel_run(batch, mu, 10)
        inclusive.append(time.perf_counter() - t0)
    n_model = min(S, 256)
    packs = [make_snowpack(thick[s], "exponential", density=dens[s], temperature=temp[s], corr_length=1e-4) for s in range(n_model)]
    model = make_model("nonscattering", "multifresnel_thermalemission")
    sensor = sensor_list.passive(FREQUENCY, THETA)
    model.run(sensor, packs)
    t_model = []
    for _ in range(3):
        t0 = time.perf_counter()
        res = model.run(sensor, packs)
        t_model.append(time.perf_counter() - t0)
    # the same layers through dort on the device
    n_dort = min(S, dort_pairs)
    dort_batch = PackedBatch([L] * n_dort, thick[:n_dort], dens[:n_dort] / 916.7, temp[:n_dort], np.full((n_dort, L), 1e-4), None,
                             [FREQUENCY], np.deg2rad(THETA), emmodel="nonscattering", microstructure="exponential",
                             n_max_stream=DORT_STREAMS)
    dort = {"pairs": n_dort, "n_max_stream": DORT_STREAMS}
    try:
        if L > DORT_MAX_LAYERS:
            raise RuntimeError("not run: more than %d layers (dort was never taken to this depth)" % DORT_MAX_LAYERS)
        ctx.run(dort_batch)
        t_dort = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref = ctx.run(dort_batch)
            t_dort.append(time.perf_counter() - t0)
        ok = ref.status == 0
        dort.update(h2d_d2h_inclusive_solves_per_s=n_dort / float(np.median(t_dort)), kernel_ms=ctx.last_kernel_ms(),
                    failed_solves=int((~ok).sum()),
                    largest_gap_K=float(np.abs(np.moveaxis(ref.values[ok], 1, 2) - out.values[:n_dort][ok]).max()) if ok.any() else None)
    except Exception as e:   # (a shape dort does not take or is not run at: reported, not hidden)
        dort["error"] = str(e)
    ms = np.asarray(layers_ms) + np.asarray(chain_ms)
    print(json.dumps({
        "metric": "snowpack x frequency multi-Fresnel solves/sec (%d layers, %d angles, 1.4 GHz)" % (L, len(THETA)),
        "value": S / float(np.median(ms)) * 1e3, "unit": "solves/s", "pairs": S, "layers": L, "n_gpus": 1, "steps": steps, "warmup": warmup,
        "kernel_ms": {"layers": spread(layers_ms), "chain": spread(chain_ms), "launch_and_sync_wall": spread(wall)},
        "layer_angle_items_per_s": S * L * len(THETA) / float(np.median(chain_ms)) * 1e3,
        "h2d_d2h_inclusive_solves_per_s": S / float(np.median(inclusive)),
        "model_run_solves_per_s": n_model / float(np.median(t_model)), "model_run_snowpacks": n_model,
        "failed_elements": int((out.status != 0).sum()), "tau_snowpack_mean": float(out.tau_snowpack.mean()),
        "dort": dort, "dtype": "f64", "data": "synthetic"}))
ctx.close()
