#!/usr/bin/env python
"""Fixtures of the successive-order backscatter solver (active mode).  RUNS ONLY IN THE BUILD CONTAINER (needs the reference
package, like make_golden.py), with the stand-ins of tests/golden/_refstubs for xarray and numba, like
make_successive_order_fixtures.py.

For every case of tests/successive_order_active_restatement.py:CASES it runs the reference's SuccessiveOrder on an active
sensor in this process and stores, as tests/golden/successive_order_active_<name>.npz: the [3, 3, n_theta_inc, order + 1]
array, the layer scalars, the per-layer sublayer and stream counts, and per pass (the coherent pass first, then the modes,
NaN-padded to the order cap) the largest emerging radiance of every order run.  It fails unless
  * at least one mode pass of some fixture stops by tolerance and at least one fixture has every pass at the cap,
  * no ratio largest emerging radiance / tolerance of any mode-pass order lies in [0.99, 1.01],
  * one fixture has layers with different stream counts,
  * one fixture has a layer with 1 sublayer and one has a layer with more than 16,
  * one fixture has a nonzero entry at an order after a stop.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_successive_order_active_fixtures.py
"""
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "_refstubs"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

warnings.filterwarnings("ignore")

from smrt import make_model, make_snowpack, make_soil, sensor_list  # noqa: E402
from smrt.rtsolver.successive_order import SuccessiveOrder  # noqa: E402

from successive_order_active_restatement import CASES, build_snowpack, solver_options  # noqa: E402

API = types.SimpleNamespace(make_snowpack=make_snowpack, make_soil=make_soil)


class Recording(SuccessiveOrder):
    """The reference's solver, unchanged, with three of its intermediate numbers written down."""

    log = None

    def prepare_layer_properties(self, *args, **kwargs):
        out = super().prepare_layer_properties(*args, **kwargs)
        self.log["sublayers"].append(int(out[0]))
        return out

    def compute_next_order(self, order, *args, **kwargs):
        profile, emerging = super().compute_next_order(order, *args, **kwargs)
        if order == 0:
            self.log["passes"].append([])
        self.log["passes"][-1].append(float(np.max(emerging[0:3 * self.streams.n_air])))
        self.log["streams"] = [int(k) for k in self.streams.n]
        return profile, emerging


def main():
    stopped, capped, refraction, one, deep, remainder = [], [], [], [], [], []
    for case in CASES:
        sp = build_snowpack(case, API)
        Recording.log = dict(sublayers=[], passes=[], streams=None)
        model = make_model(case["emmodel"], Recording, rtsolver_options=solver_options(case))
        res = model.run(sensor_list.active(case["frequency"], case["theta"]), sp, parallel_computation="none")
        log = Recording.log
        sigma = np.asarray(res.data.values, float)
        n_it, m_max = case["n_iteration_max"], case.get("m_max", 2)
        assert sigma.shape == (3, 3, len(case["theta"]), n_it + 1), sigma.shape
        passes = log["passes"]
        assert len(passes) == m_max + 2 and len(passes[0]) == n_it, [len(p) for p in passes]
        tolerance = case.get("relative_tolerance", 0.001) * passes[1][0]
        pass_max = np.full((m_max + 2, n_it), np.nan)
        for k, p in enumerate(passes):
            pass_max[k, :len(p)] = p
            if k > 0 and tolerance > 0:
                ratio = np.array(p) / tolerance
                assert not np.any((ratio >= 0.99) & (ratio <= 1.01)), (case["name"], k, ratio)
        ran = [len(p) for p in passes[1:]]
        if any(r < n_it or passes[1 + k][-1] < tolerance for k, r in enumerate(ran)):
            stopped.append(case["name"])
        else:
            capped.append(case["name"])
        if min(ran) < n_it and np.any(sigma[:, :, :, min(ran):n_it] != 0.0):
            remainder.append(case["name"])
        streams, sublayers = log["streams"], log["sublayers"]
        if len(set(streams)) > 1:
            refraction.append(case["name"])
        if min(sublayers) == 1:
            one.append(case["name"])
        if max(sublayers) > 16:
            deep.append(case["name"])
        other = res.other_data
        np.savez(os.path.join(HERE, "successive_order_active_" + case["name"] + ".npz"), sigma=sigma,
                 eps=np.asarray(other["effective_permittivity"].values, complex), ks=np.asarray(other["ks"].values, float),
                 ka=np.asarray(other["ka"].values, float), sublayers=np.array(sublayers), streams=np.array(streams),
                 pass_max=pass_max)
        print(case["name"], "orders run per mode:", ran, "VV total:", sigma[0, 0, :, -1], "order 1:", sigma[0, 0, :, 1],
              "sublayers:", sublayers, "streams:", streams)
    print("a mode pass stopped by tolerance:", stopped, "\nevery pass at the cap:", capped, "\ndifferent stream counts:", refraction,
          "\na layer of 1 sublayer:", one, "\na layer of more than 16:", deep, "\nnonzero after a stop:", remainder)
    assert stopped and capped and refraction and one and deep and remainder


if __name__ == "__main__":
    main()
