#!/usr/bin/env python
"""Fixtures of the successive-order solver.  RUNS ONLY IN THE BUILD CONTAINER (needs the reference package, like
make_golden.py), with the stand-ins of tests/golden/_refstubs for xarray and numba, like make_first_order_fixtures.py.

For every case of tests/successive_order_restatement.py:FIXTURE_CASES (the cases without a substrate) it runs the reference's
SuccessiveOrder in this process and stores, as tests/golden/successive_order_<name>.npz: the [pol, theta, order + 1] array in
kelvin, the layer scalars, the per-layer sublayer and stream counts and the largest emerging radiance of every order run
(the inputs are the case table itself).  It fails unless
  * at least one fixture stops by tolerance and at least one hits the order cap,
  * for every order run the ratio largest emerging radiance / tolerance lies outside [0.99, 1.01] (the stopping decision
    must not hang on rounding),
  * at least one fixture has layers with different stream counts,
  * at least one fixture has a layer with 1 sublayer and one with more than 16.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_successive_order_fixtures.py
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
from smrt.substrate.reflector import make_reflector  # noqa: E402

from successive_order_restatement import FIXTURE_CASES, build_snowpack, solver_options  # noqa: E402

API = types.SimpleNamespace(make_snowpack=make_snowpack, make_soil=make_soil, make_reflector=make_reflector)


class Recording(SuccessiveOrder):
    """The reference's solver, unchanged, with three of its intermediate numbers written down."""

    log = None

    def prepare_layer_properties(self, *args, **kwargs):
        out = super().prepare_layer_properties(*args, **kwargs)
        self.log["sublayers"].append(int(out[0]))
        return out

    def compute_next_order(self, *args, **kwargs):
        profile, emerging = super().compute_next_order(*args, **kwargs)
        self.log["max_radiance"].append(float(np.max(emerging[0:2 * self.streams.n_air])))
        self.log["streams"] = [int(k) for k in self.streams.n]
        return profile, emerging


def main():
    stopped, capped, refraction, one, deep = [], [], [], [], []
    for case in FIXTURE_CASES:
        sp = build_snowpack(case, API)
        options = solver_options(case)
        if "reference_m_max" in case:
            options["m_max"] = case["reference_m_max"]
        Recording.log = dict(sublayers=[], max_radiance=[], streams=None)
        model = make_model(case["emmodel"], Recording, rtsolver_options=options)
        try:
            res = model.run(sensor_list.passive(case["frequency"], case["theta"]), sp, parallel_computation="none")
        except Exception as e:   # (dmrt_L2_n8 was not tried when the case table was written)
            print(case["name"], "NOT PRODUCED by the reference:", type(e).__name__, e)
            continue
        log = Recording.log
        tb = np.asarray(res.data.values, float)
        n_it = case["n_iteration_max"]
        assert tb.shape == (2, len(case["theta"]), n_it + 1), tb.shape
        radiance = np.array(log["max_radiance"])
        rtol = case.get("relative_tolerance", 0.001)
        tolerance = rtol * radiance[0]
        if tolerance > 0:
            ratio = radiance / tolerance
            assert not np.any((ratio >= 0.99) & (ratio <= 1.01)), (case["name"], ratio)
        (capped if len(radiance) == n_it and not radiance[-1] < tolerance else stopped).append(case["name"])
        assert np.all(tb[:, :, len(radiance):n_it] == 0.0), case["name"]
        streams, sublayers = log["streams"], log["sublayers"]
        if len(set(streams)) > 1:
            refraction.append(case["name"])
        if min(sublayers) == 1:
            one.append(case["name"])
        if max(sublayers) > 16:
            deep.append(case["name"])
        other = res.other_data
        np.savez(os.path.join(HERE, "successive_order_" + case["name"] + ".npz"), tb=tb,
                 eps=np.asarray(other["effective_permittivity"].values, complex), ks=np.asarray(other["ks"].values, float),
                 ka=np.asarray(other["ka"].values, float), sublayers=np.array(sublayers), streams=np.array(streams),
                 max_radiance=radiance)
        print(case["name"], "orders run:", len(radiance), "TbV total:", np.round(tb[0, :, -1], 4), "order 0:", np.round(tb[0, :, 0], 4),
              "sublayers:", sublayers, "streams:", streams)
    print("stopped by tolerance:", stopped, "\nhit the cap:", capped, "\ndifferent stream counts:", refraction,
          "\na layer of 1 sublayer:", one, "\na layer of more than 16:", deep)
    assert stopped and capped and refraction and one and deep


if __name__ == "__main__":
    main()
