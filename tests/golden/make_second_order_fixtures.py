#!/usr/bin/env python
"""Fixtures of the iterative second-order solver.  RUNS ONLY IN THE BUILD CONTAINER (needs the reference package, like
make_golden.py), with the stand-ins of tests/golden/_refstubs for xarray and numba, like make_first_order_fixtures.py.

For every case of tests/second_order_restatement.py:CASES it runs the reference's IterativeSecondOrder with
return_contributions=True and stores, as tests/golden/second_order_<name>.npz: the 8 contributions, backscatter_layer and
the layer scalars (the inputs are the case table itself).  It fails unless each of the three order-2 mechanisms exceeds
1 % of the largest co-polarised total in at least one case, unless HV of the total is non-zero wherever a layer scatters,
and unless at least one interlayer value is negative (the finding of DESIGN.md section 4f).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_second_order_fixtures.py [NAME ...]

With names only those cases are run and written (the conditions on the whole set are then not checked).
"""
import contextlib
import io
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

from second_order_restatement import CASES, CONTRIBUTIONS, build_snowpack, options_of  # noqa: E402

# the reference's solve() fails on a substrate whose permittivity has no imaginary part (it appends to an array): the
# transparent substrate, which never reads its permittivity, gets a token one
API = types.SimpleNamespace(make_snowpack=make_snowpack, make_interface=make_interface, make_soil=make_soil,
                            make_reflector=make_reflector,
                            transparent_substrate=lambda: make_soil("transparent", complex(1.0, 1e-6), 270.0))


def main(names=()):
    largest_share = np.zeros(3)
    most_negative = 0.0
    unknown = set(names) - {c["name"] for c in CASES}
    assert not unknown, f"no such case: {sorted(unknown)}"
    for case in CASES:
        if names and case["name"] not in names:
            continue
        sp = build_snowpack(case, API)
        model = make_model(case["emmodel"], "iterative_second_order", rtsolver_options=dict(return_contributions=True, **options_of(case)))
        with contextlib.redirect_stdout(io.StringIO()):   # the reference's geometrical optics prints on every call
            res = model.run(sensor_list.active(case["frequency"], case["theta"]), sp)
        data = np.asarray(res.data.values, float)
        assert data.shape == (8, len(case["theta"]), 2, 2)
        other = res.other_data
        layer = np.asarray(other["backscatter_layer"].values, float)
        assert layer.shape == (len(case["thickness"]) + 1, len(case["theta"]), 2, 2)
        copol = max(data[0, :, 0, 0].max(), data[0, :, 1, 1].max())
        shares = [max(data[5 + c, :, 0, 0].max(), data[5 + c, :, 1, 1].max()) / copol for c in range(3)]
        largest_share = np.maximum(largest_share, shares)
        most_negative = min(most_negative, data[7].min())
        ks = np.asarray(other["ks"].values, float)
        if ks.max() > 0:
            assert np.all(data[0, :, 0, 1] != 0.0) and np.all(data[0, :, 1, 0] != 0.0), case["name"]
        np.savez(os.path.join(HERE, "second_order_" + case["name"] + ".npz"), contributions=data, backscatter_layer=layer,
                 eps=np.asarray(other["effective_permittivity"].values, complex), ks=ks, ka=np.asarray(other["ka"].values, float))
        print(case["name"], "sigmaVV dB:", np.round(10 * np.log10(4 * np.pi * np.cos(np.deg2rad(case["theta"])) * data[0, :, 0, 0]), 3),
              "order-2 shares:", np.round(shares, 4), "HV/VV:", np.round(data[0, :, 0, 1] / data[0, :, 0, 0], 4))
    if names:
        return
    print("largest share of the total per order-2 mechanism:", dict(zip(CONTRIBUTIONS[5:], np.round(largest_share, 4))))
    print("most negative interlayer value:", most_negative)
    assert np.all(largest_share > 0.01), "every order-2 mechanism must exceed 1 % of the total in at least one fixture"
    assert most_negative < 0.0, "no negative interlayer value: the finding is not pinned"


if __name__ == "__main__":
    main(sys.argv[1:])
