#!/usr/bin/env python
"""Fixtures of the multi-Fresnel thermal emission solver.  RUNS ONLY IN THE BUILD CONTAINER (needs the reference package, like
make_golden.py), with the stand-ins of tests/golden/_refstubs for xarray and numba, like make_successive_order_fixtures.py.

For every case of tests/multifresnel_restatement.py:CASES it runs the reference's MultiFresnelThermalEmission in this process
and stores, as tests/golden/multifresnel_<name>.npz: tb [theta, pol], the layer scalars, the number of layer matrices the
reference multiplied (layers_used), its tau_snowpack and, per angle, the index of the first layer whose optical depth was
clipped (-1 if none); the inputs are the case table itself.  Every file is written first; then the script FAILS unless
  1. at least one case stops before its last layer,
  2. at least one case has an angle clipped to zero for one or more layers before the stop,
  3. at least one case never clips,
  4. in every case, every value of the steepest angle's tau_remaining that decides a stop is farther than 1e-9 from 0,
  5. all values are finite.

RECORDED OUTCOME (see tests/multifresnel_restatement.py and DESIGN.md 4e): 2, 3 and 5 hold; 1 and 4 cannot hold with this
reference.  Its stop needs tau_remaining < 0 and tau_remaining is x - clip(tau, 0, x) >= 0: the stop never fires, and once the
steepest angle is exhausted the deciding value is exactly 0 (firn_prune1).  No frequency or depth changes that.  The script
therefore exits with a failure that names 1 and 4, after writing fixtures that are the reference's results all the same.
With prune_deep_snowpack=None the reference clips against NaN and returns NaN everywhere; `firn_noprune` is the reference at
prune_deep_snowpack=inf, which is the computation without clipping (and the script checks that None does give NaN).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_multifresnel_fixtures.py
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
from smrt.rtsolver.multifresnel import multifresnel as reference_chain  # noqa: E402

from multifresnel_restatement import CASES, build_snowpack, solver_options  # noqa: E402

API = types.SimpleNamespace(make_snowpack=make_snowpack, make_soil=make_soil)
LOG = []
_forward = reference_chain.forward_matrix_fulloutput


def recording_forward(*args, **kwargs):
    """The reference's layer matrix, unchanged, with its limit and optical depths written down."""
    out = _forward(*args, **kwargs)
    mu = np.atleast_1d(args[2])
    raw = 2 * np.sqrt(complex(args[1])).imag * kwargs["kd"] / out[1][0]
    LOG.append(dict(limit=np.array(kwargs["limit_optical_depth"], float), tau=np.array(out[1][1], float), raw=raw, mu=mu))
    return out


reference_chain.forward_matrix_fulloutput = recording_forward


def run(case, options):
    del LOG[:]
    model = make_model(case["emmodel"], "multifresnel_thermalemission", rtsolver_options=options)
    res = model.run(sensor_list.passive(case["frequency"], case["theta"]), build_snowpack(case, API), parallel_computation="none")
    return res, [dict(e) for e in LOG]


def main():
    stops, zeroed, unclipped, near_zero, nonfinite = [], [], [], [], []
    for case in CASES:
        options = solver_options(case)
        if "prune_deep_snowpack" in options and options["prune_deep_snowpack"] is None:
            res, _ = run(case, options)
            assert np.all(np.isnan(res.data.values)), "the reference with prune_deep_snowpack=None no longer gives NaN: revisit"
            options = dict(prune_deep_snowpack=np.inf)
        res, log = run(case, options)
        tb = np.asarray(res.data.values, float)
        assert res.data.dims == ("theta", "polarization") and tb.shape == (len(case["theta"]), 2), (res.data.dims, tb.shape)
        steepest = int(np.argmax(np.cos(np.deg2rad(case["theta"]))))
        n_slots = res.other_data["ks"].values.shape[0] + (1 if "substrate" in case else 0)
        tau = np.array([e["tau"] for e in log])          # [layers used, theta]
        raw = np.array([e["raw"] for e in log])
        clipped = tau < raw
        first_clipped = np.where(clipped.any(axis=0), clipped.argmax(axis=0), -1)
        deciding = np.array([e["limit"][steepest] - e["tau"][steepest] for e in log])
        tau_snowpack = float(sum(e["tau"][steepest] for e in log))
        if len(log) < n_slots:
            stops.append(case["name"])
        if np.any((tau == 0.0) & (raw > 0.0)):
            zeroed.append(case["name"])
        if not clipped.any():
            unclipped.append(case["name"])
        if np.any(np.abs(deciding) <= 1e-9):
            near_zero.append(case["name"])
        other = res.other_data
        arrays = dict(tb=tb, eps=np.asarray(other["effective_permittivity"].values, complex), ks=np.asarray(other["ks"].values, float),
                      ka=np.asarray(other["ka"].values, float), layers_used=np.array(len(log)), tau_snowpack=np.array(tau_snowpack),
                      first_clipped=first_clipped)
        if not all(np.all(np.isfinite(a)) for a in arrays.values()):
            nonfinite.append(case["name"])
        np.savez(os.path.join(HERE, "multifresnel_" + case["name"] + ".npz"), **arrays)
        print(case["name"], "Tb V:", np.round(tb[:, 0], 4), "H:", np.round(tb[:, 1], 4), "layers used:", len(log), "of", n_slots,
              "tau_snowpack: %.6g" % tau_snowpack, "first clipped:", first_clipped, "smallest |deciding remainder|: %.3g" % np.abs(deciding).min())
    print("1. stops before the last layer:", stops, "\n2. an angle clipped to zero:", zeroed, "\n3. never clips:", unclipped,
          "\n4. a deciding remainder within 1e-9 of 0:", near_zero, "\n5. non-finite:", nonfinite)
    failed = [k for k, ok in ((1, stops), (2, zeroed), (3, unclipped), (4, not near_zero), (5, not nonfinite)) if not ok]
    assert not failed, "conditions not met: %s" % failed


if __name__ == "__main__":
    main()
