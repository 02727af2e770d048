#!/usr/bin/env python
"""Fixtures of the soil substrates (Wegmuller, QNH, Choudhury) and of the soil / bedrock permittivities.  RUNS ONLY IN THE
BUILD CONTAINER (needs the reference package, like make_golden.py), with the stand-ins of tests/golden/_refstubs for xarray
and numba.  Writes

  soil_wegmuller_<model>.npz   the three snow-on-soil cases of smrt/test/test_soil.py (DMRT-QCA-CP, 2 layers, 37 GHz, 40
                               degrees; Wegmuller soil on Dobson-Peplinski, Dobson-original, Montpetit08).  The reference's own
                               constants are asserted here at its own 1e-4.
  soil_edge.npz                IBA exponential, 19 and 37 GHz, three 2-layer snowpacks whose bottom layer is less dense than
                               the top one, on Wegmuller, QNH and Choudhury soil, all soil parameters different; viewing angles
                               25, 55, 70 degrees.  DORT at n_max_stream 8, 34 and 66, successive_order at 8 and 34, and what
                               the three substrate classes return on the streams of the last layer (n_max_stream 8).
  soil_permittivity_table.npz  the four soil models at ten points and every bedrock model at two frequencies.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_soil_fixtures.py
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "_refstubs"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

warnings.filterwarnings("ignore")

from smrt import make_model, make_snowpack, sensor_list  # noqa: E402
from smrt.inputs.make_soil import make_soil_substrate  # noqa: E402
from smrt.permittivity import bedrock as ref_bedrock, soil as ref_soil  # noqa: E402

from soil_cases import (BEDROCK_FREQUENCIES, EDGE, EDGE_SO_OPTIONS, PERMITTIVITY_POINTS, SOIL_MODELS, WEGMULLER_CASES,  # noqa: E402
                        WEGMULLER_SNOW, last_layer_streams)


def tb_of(res):
    """[V | H][theta] of a passive result (the stand-in of xarray has no .sel)."""
    data, dims = np.asarray(res.data.values, float), tuple(res.data.dims)
    assert set(dims) == {"theta", "polarization"}, dims
    return data if dims == ("polarization", "theta") else data.T   # (V before H: the constants asserted below pin the order)


def wegmuller_cases():
    for model, (tbv, tbh) in WEGMULLER_CASES.items():
        soil = dict(WEGMULLER_SNOW["soil"]) if model != "soil_permittivity_montpetit08" else {}
        substrate = make_soil_substrate("soil_wegmuller", model, WEGMULLER_SNOW["soil_temperature"],
                                        roughness_rms=WEGMULLER_SNOW["roughness_rms"], **soil)
        sp = make_snowpack(WEGMULLER_SNOW["thickness"], "sticky_hard_spheres", density=WEGMULLER_SNOW["density"],
                           temperature=WEGMULLER_SNOW["temperature"], radius=WEGMULLER_SNOW["radius"],
                           stickiness=WEGMULLER_SNOW["stickiness"], substrate=substrate)
        res = make_model("dmrt_qcacp_shortrange", "dort").run(sensor_list.passive(37e9, 40), sp)
        v, h = (float(x) for x in tb_of(res)[:, 0])
        assert abs(v - tbv) < 1e-4 and abs(h - tbh) < 1e-4, (model, v, h)
        np.savez(os.path.join(HERE, "soil_wegmuller_" + model[len("soil_permittivity_"):] + ".npz"), tb=np.array([v, h]),
                 eps_soil=complex(substrate.permittivity(37e9)))
        print(model, v, h)


def edge_substrate(k):
    spec = EDGE["substrates"][k]
    return make_soil_substrate(spec["model"], spec["permittivity_model"], spec["temperature"], **spec["soil"], **spec["parameters"])


def edge_snowpack(k):
    snow = EDGE["snow"][k]
    return make_snowpack(snow["thickness"], "exponential", density=snow["density"], temperature=snow["temperature"],
                         corr_length=snow["corr_length"], substrate=edge_substrate(k))


def soil_edge():
    F, S, T = len(EDGE["frequency"]), len(EDGE["snow"]), len(EDGE["theta"])
    out = {}
    for n in (8, 34, 66):
        tb = np.empty((F, S, 2, T))
        for fi, f in enumerate(EDGE["frequency"]):
            for s in range(S):
                res = make_model("iba", "dort", rtsolver_options=dict(n_max_stream=n)).run(sensor_list.passive(f, EDGE["theta"]), edge_snowpack(s))
                tb[fi, s] = tb_of(res)
                if n == 8:
                    eps = np.asarray(res.other_data["effective_permittivity"].values, complex)
                    out.setdefault("eps_layers", np.empty((F, S, 2), complex))[fi, s] = eps
        out["dort_n%d" % n] = tb
        print("dort n_max_stream", n, "TbV:", np.round(tb[:, :, 0], 4).tolist())
    for n in (8, 34):
        options = dict(EDGE_SO_OPTIONS, n_max_stream=n)
        tb = np.empty((F, S, 2, T, options["n_iteration_max"] + 1))
        for fi, f in enumerate(EDGE["frequency"]):
            for s in range(S):
                res = make_model("iba", "successive_order", rtsolver_options=options).run(sensor_list.passive(f, EDGE["theta"]), edge_snowpack(s),
                                                                                            parallel_computation="none")
                tb[fi, s] = np.asarray(res.data.values, float)
        out["successive_order_n%d" % n] = tb
        print("successive_order n_max_stream", n, "TbV total:", np.round(tb[:, :, 0, :, -1], 4).tolist())
    # the protocol of the three classes on the streams of the last layer (n_max_stream = 8): both sides of 60 degrees, fewer
    # streams than n_max_stream
    for fi, f in enumerate(EDGE["frequency"]):
        for s in range(S):
            eps = out["eps_layers"][fi, s]
            mu = last_layer_streams(eps, 8)
            angles = np.degrees(np.arccos(mu))
            assert len(mu) < 8 and angles.min() < 60 < angles.max(), (f, s, angles)
            sub = edge_substrate(s)
            for npol in (2, 3):
                out["spec_f%d_s%d_npol%d" % (fi, s, npol)] = np.asarray(sub.specular_reflection_matrix(f, eps[-1], mu.copy(), npol).values, float)
                out["emis_f%d_s%d_npol%d" % (fi, s, npol)] = np.asarray(sub.emissivity_matrix(f, eps[-1], mu.copy(), npol).values, float)
            out["mu_f%d_s%d" % (fi, s)] = mu
            out.setdefault("eps_soil", np.empty((F, S), complex))[fi, s] = complex(sub.permittivity(f))
    np.savez(os.path.join(HERE, "soil_edge.npz"), **out)


def permittivity_table():
    out = {}
    for name, arguments in SOIL_MODELS.items():
        function = getattr(ref_soil, name)
        values = []
        for point in PERMITTIVITY_POINTS[name]:
            sub = make_soil_substrate("flat", function, point["temperature"], **{a: point[a] for a in arguments if a != "temperature"})
            values.append(complex(sub.permittivity(point["frequency"])))
        out[name] = np.array(values)
    names = sorted(n for n in dir(ref_bedrock) if n.startswith("bedrock_permittivity_"))
    out["bedrock_names"] = np.array(names)
    out["bedrock"] = np.array([[complex(make_soil_substrate("flat", getattr(ref_bedrock, n), 270).permittivity(f)) for f in BEDROCK_FREQUENCIES]
                               for n in names])
    np.savez(os.path.join(HERE, "soil_permittivity_table.npz"), **out)
    print("permittivities:", {k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    permittivity_table()
    wegmuller_cases()
    soil_edge()
