#!/usr/bin/env python
"""Model.run on snowpacks with a rough surface, the device route (rough boundaries evaluated by the builder kernels,
smrt_amd/csrc/rough_boundary_kernel.hpp) against the dense host route of the same objects (Python evaluates the interface per
pair and hands over dense matrices -- the only route before the builder existed, unchanged since).  Two workloads of 3-layer
snowpacks at one frequency:

  go_active     a geometrical_optics surface, active, 16 streams, m_max 2
  iem_passive   an iem_fung92 surface, passive, 32 streams

Prints ONE JSON line: per workload the solves/s of Model.run on both routes (median of `reps` runs after one warm-up; the host
route on `host_snowpacks` of the snowpacks, it is slow), their ratio, the builder kernels' own HIP-event time and the bytes of
matrices they built.  No rate is a gate.
   python tools/bench_rough_boundaries.py [snowpacks] [host_snowpacks] [reps]"""
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from smrt_amd import make_interface, make_model, make_snowpack, sensor_list  # noqa: E402
from smrt_amd.rtsolver.dort import get_context  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 256
host_snowpacks = int(sys.argv[2]) if len(sys.argv) > 2 else 32
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3


class HostRoute:
    """The same interface without its device_kind: evaluated in Python per pair."""

    def __init__(self, target):
        self._target = target

    def __getattr__(self, name):
        if name in ("device_kind", "device_params", "_target"):
            raise AttributeError(name)
        return getattr(self._target, name)


rng = np.random.default_rng(11)
columns = [dict(thickness=[rng.uniform(0.1, 0.4), rng.uniform(0.2, 0.8), 10.0], density=list(rng.uniform(200, 400, 3)),
                temperature=list(rng.uniform(250, 268, 3)), corr_length=list(rng.uniform(8e-5, 3e-4, 3))) for _ in range(S)]


def packs(interface, wrap, n):
    return [make_snowpack(c["thickness"], "exponential", density=c["density"], temperature=c["temperature"], corr_length=c["corr_length"],
                          interface=[wrap(interface(k)), "flat", "flat"]) for k, c in enumerate(columns[:n])]


def rate(model, sensor, snowpacks):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.run(sensor, snowpacks)
        seconds = []
        for _ in range(reps):
            t0 = time.perf_counter()
            model.run(sensor, snowpacks)
            seconds.append(time.perf_counter() - t0)
    return len(snowpacks) / float(np.median(seconds))


def workload(interface, model, sensor):
    device = rate(model, sensor, packs(interface, lambda o: o, S))
    info = get_context().rough_info()
    host = rate(model, sensor, packs(interface, HostRoute, host_snowpacks))
    return {"device_route_solves_per_s": device, "device_route_snowpacks": S, "host_route_solves_per_s": host,
            "host_route_snowpacks": host_snowpacks, "ratio": device / host, "builder_kernels_ms": info["builder_ms"],
            "built_bytes": info["built_bytes"], "host_matrix_bytes_on_the_device_route": info["host_matrix_bytes"]}


slopes = rng.uniform(0.02, 0.08, S)
heights = rng.uniform(1e-3, 3e-3, S)
out = {
    "go_active": workload(lambda k: make_interface("geometrical_optics", mean_square_slope=slopes[k]),
                          make_model("iba", "dort", rtsolver_options=dict(n_max_stream=16, m_max=2)), sensor_list.active(13.4e9, 40.0)),
    "iem_passive": workload(lambda k: make_interface("iem_fung92", roughness_rms=heights[k], corr_length=0.05),
                            make_model("iba", "dort", rtsolver_options=dict(n_max_stream=32)), sensor_list.passive(36.5e9, 55.0)),
}
print(json.dumps({"metric": "Model.run solves/s on 3-layer snowpacks with a rough surface, device route against dense host route",
                  "value": out["go_active"]["device_route_solves_per_s"], "unit": "solves/s", "n_gpus": 1, "reps": reps, "workloads": out,
                  "dtype": "f64", "data": "synthetic"}))
