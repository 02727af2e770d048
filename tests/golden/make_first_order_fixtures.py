#!/usr/bin/env python
"""Fixtures of the iterative first-order solver.  RUNS ONLY IN THE BUILD CONTAINER (needs the reference package, like
make_golden.py), with the stand-ins of tests/golden/_refstubs for xarray and numba, like make_golden.py.

For every case of tests/first_order_restatement.py:CASES it runs the reference's IterativeFirstOrder with
return_contributions=True and stores, as tests/golden/first_order_<name>.npz: the 5 contributions, backscatter_layer and the
layer scalars (the inputs are the case table itself).  It fails unless each of the four mechanisms exceeds 1 % of the
total co-polarised backscatter in at least one case, and unless order 0 is exactly zero with Flat interfaces off nadir.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_first_order_fixtures.py
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

from smrt import make_interface, make_model, make_snowpack, make_soil, sensor_list  # noqa: E402
from smrt.substrate.reflector import make_reflector  # noqa: E402

from first_order_restatement import CASES, CONTRIBUTIONS  # noqa: E402

API = types.SimpleNamespace(make_snowpack=make_snowpack, make_interface=make_interface, make_soil=make_soil,
                            make_reflector=make_reflector, transparent_substrate=lambda: make_soil("transparent", 1.0, 270.0))


def main():
    from first_order_restatement import build_snowpack

    largest_share = np.zeros(4)
    for case in CASES:
        sp = build_snowpack(case, API)
        model = make_model(case["emmodel"], "iterative_first_order", rtsolver_options=dict(return_contributions=True))
        res = model.run(sensor_list.active(case["frequency"], case["theta"]), sp)
        data = np.asarray(res.data.values, float)
        assert data.shape == (5, len(case["theta"]), 2, 2)
        other = res.other_data
        layer = np.asarray(other["backscatter_layer"].values, float)
        assert layer.shape == (len(case["thickness"]) + 1, len(case["theta"]), 2, 2)
        copol = max(data[0, :, 0, 0].max(), data[0, :, 1, 1].max())
        for c in range(4):
            largest_share[c] = max(largest_share[c], max(data[1 + c, :, 0, 0].max(), data[1 + c, :, 1, 1].max()) / copol)
        if not case.get("interfaces") and case.get("substrate", {}).get("substrate_model", "flat") == "flat" \
                and "transparent" not in case.get("substrate", {}):
            assert np.all(data[1] == 0.0), case["name"]   # Flat everywhere, off nadir: no order-0 return at all
        np.savez(os.path.join(HERE, "first_order_" + case["name"] + ".npz"), contributions=data, backscatter_layer=layer,
                 eps=np.asarray(other["effective_permittivity"].values, complex), ks=np.asarray(other["ks"].values, float),
                 ka=np.asarray(other["ka"].values, float))
        print(case["name"], "sigmaVV dB:", np.round(10 * np.log10(4 * np.pi * np.cos(np.deg2rad(case["theta"])) * data[0, :, 0, 0]), 3),
              "shares:", np.round([data[1 + c, :, 0, 0].max() / copol for c in range(4)], 4))
    print("largest share of the total per mechanism:", dict(zip(CONTRIBUTIONS[1:], np.round(largest_share, 4))))
    assert np.all(largest_share > 0.01), "every mechanism must exceed 1 % of the total in at least one fixture"


if __name__ == "__main__":
    main()
