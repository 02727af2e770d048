#!/usr/bin/env python
"""Throughput of DORT on snow over Wegmuller soil at the headline shape (bench.py configs[1]: IBA, 20 layers, 32 streams, five
AMSR-E channels at 55 degrees, 1024 synthetic snowpacks = 5120 solves per launch; every snowpack on its own soil).  Prints ONE
JSON line:

  resident            solves/s of the launch alone, inputs in HBM (median wall time of `steps` launches after `warmup`): on
                      Wegmuller soil, on a Flat substrate of the same permittivities and without a substrate -- same command,
                      same batch, only the substrate kind differs
  model_run           solves/s of Model.run on the soil snowpacks (packing, soil permittivities, H2D, launch, D2H, results)
  dense_host_route    the same snowpacks, `host_snowpacks` of them, with the soil behind a stand-in that has no device_kind:
                      Python evaluates the substrate per pair and hands over dense reflection matrices (SMRT_SUBSTRATE_HOST)

No rate is a gate.
   python tools/bench_soil.py [steps] [warmup] [host_snowpacks]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import FREQS, N_LAYERS, N_SNOWPACKS, N_STREAMS, THETA_DEG, synthetic_snowpacks  # noqa: E402
from smrt_amd import make_model, make_snowpack, make_soil, sensor_list  # noqa: E402
from smrt_amd._native import DortContext, PackedBatch  # noqa: E402
from smrt_amd.core.substrate import batch_permittivities  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
host_snowpacks = int(sys.argv[3]) if len(sys.argv) > 3 else 32


class HostRoute:
    """The same soil without its device_kind: evaluated in Python per pair."""

    def __init__(self, substrate):
        self.substrate, self.temperature = substrate, substrate.temperature

    def specular_reflection_matrix(self, *args):
        return self.substrate.specular_reflection_matrix(*args)

    def emissivity_matrix(self, *args):
        return self.substrate.emissivity_matrix(*args)


def resident_rate(ctx, batch):
    ctx.upload(batch)
    for _ in range(warmup):
        ctx.launch()
    ctx.sync()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        ctx.launch()
        ctx.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    failed = int((ctx.download().status != 0).sum())
    return {"solves_per_s": batch.n_pairs / float(np.median(ms)) * 1e3, "ms_per_launch": {"median": float(np.median(ms)), "min": float(min(ms)),
            "max": float(max(ms))}, "failed_solves": failed}


rng = np.random.default_rng(7)
S = N_SNOWPACKS
thick, dens, temp, lc = synthetic_snowpacks(seed=2, S=S)
soils = [make_soil("soil_wegmuller", "soil_permittivity_dobson85_peplinski95", rng.uniform(262, 273), moisture=rng.uniform(0.05, 0.35),
                   sand=rng.uniform(0.2, 0.6), clay=rng.uniform(0.1, 0.3), dry_matter=1100, roughness_rms=rng.uniform(2e-3, 2e-2)) for _ in range(S)]
eps = batch_permittivities(soils, FREQS)
soil_T = [soil.temperature for soil in soils]
tails = np.array([soil.device_tail() for soil in soils])


def batch(substrate):
    return PackedBatch([N_LAYERS] * S, thick, dens / 916.7, temp, lc, None, FREQS, np.deg2rad([THETA_DEG]), emmodel="iba",
                       microstructure="exponential", mode="P", n_max_stream=N_STREAMS, substrate=substrate)


ctx = DortContext(0)
resident = {"soil_wegmuller": resident_rate(ctx, batch(("soil_wegmuller", eps.real, eps.imag, soil_T, tails[:, 0], tails[:, 1]))),
            "flat": resident_rate(ctx, batch(("flat", eps.real, eps.imag, soil_T))), "no_substrate": resident_rate(ctx, batch(None))}
ctx.close()


def packs(wrap, n):
    return [make_snowpack(thick[s], "exponential", density=dens[s], temperature=temp[s], corr_length=lc[s], substrate=wrap(soils[s]))
            for s in range(n)]


def model_rate(snowpacks, reps=3):
    model = make_model("iba", "dort", rtsolver_options=dict(n_max_stream=N_STREAMS))
    sensor = sensor_list.passive(list(FREQS), THETA_DEG)
    model.run(sensor, snowpacks)
    seconds = []
    for _ in range(reps):
        t0 = time.perf_counter()
        model.run(sensor, snowpacks)
        seconds.append(time.perf_counter() - t0)
    return len(snowpacks) * len(FREQS) / float(np.median(seconds))


print(json.dumps({
    "metric": "snowpack x frequency DORT solves/sec on Wegmuller soil (20 layers, 32 streams)", "value": resident["soil_wegmuller"]["solves_per_s"],
    "unit": "solves/s", "n_gpus": 1, "steps": steps, "warmup": warmup, "solves_per_launch": S * len(FREQS), "resident": resident,
    "model_run_solves_per_s": model_rate(packs(lambda soil: soil, S)), "model_run_snowpacks": S,
    "dense_host_route_solves_per_s": model_rate(packs(HostRoute, host_snowpacks)), "dense_host_route_snowpacks": host_snowpacks,
    "dtype": "f64", "data": "synthetic"}))
