#!/usr/bin/env python
"""Fixtures of the nadir SAR altimetry solver.  RUNS ONLY WHERE THE REFERENCE PACKAGE IS (its directory in SMRT_REFERENCE, by
default next to this repository), with the stand-ins of tests/golden/_refstubs for xarray and numba, like
make_nadir_lrm_altimetry_fixtures.py.

For every case of tests/nadir_sar_altimetry_restatement.py:CASES it runs the reference's NadirSARAltimetry.solve in this process,
with return_oversampled=True (the stand-in xarray has no coarsen), and stores as tests/golden/nadir_sar_altimetry_<name>.npz: the
map per contribution and the total as the case asks for it -- oversampled, or the mean over the oversampling blocks taken here --
with the names of the contributions, delay, doppler_frequency, gate, doppler_bin, z_gate, the volume backscatter per sub-gate, the
coherent and incoherent echo of every boundary, t_interface.  sar_altimeter_list.npz holds every attribute of every sensor of the
reference's list.  `xr` and `AltimetryResult` are replaced IN THE NAMESPACE OF THE REFERENCE MODULE by a recorder; nothing of the
reference is changed on disk.

The script FAILS if the reference raises on a case or a value is not finite (z_gate below the snowpack is NaN by design).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_nadir_sar_altimetry_fixtures.py
"""
import contextlib
import io
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "_refstubs"))
sys.path.insert(0, os.environ.get("SMRT_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference")))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

warnings.filterwarnings("ignore")

from smrt import make_interface, make_model, make_snowpack, make_soil  # noqa: E402
from smrt.core.terrain import TerrainInfo  # noqa: E402
from smrt.inputs import sar_altimeter_list  # noqa: E402
from smrt.rtsolver import nadir_sar_altimetry as reference  # noqa: E402

from nadir_sar_altimetry_restatement import CASES, build_snowpack, make_sensor, solver_options  # noqa: E402

API = types.SimpleNamespace(make_snowpack=make_snowpack, make_soil=make_soil, make_interface=make_interface,
                            sar_altimeter_list=sar_altimeter_list, TerrainInfo=TerrainInfo)
SENSOR_ATTRIBUTES = ("frequency", "altitude", "pulse_bandwidth", "beamwidth_alongtrack", "beamwidth_acrosstrack", "antenna_gain", "ngate",
                     "ndoppler", "nominal_gate", "pitch_angle", "roll_angle", "off_nadir_angle", "alpha", "pulse_repetition_frequency",
                     "velocity", "wavelength", "burst_duration", "theta_inc_deg", "theta_deg", "phi_deg")


class Recorded:
    """What the reference builds its result from: values, coordinates, the coordinates it assigns, z_gate."""

    def __init__(self, values, coords=None):
        self.values = np.asarray(values)
        self.coords = [(c[0], np.asarray(c[1])) for c in coords if isinstance(c, tuple)]
        for k, v in self.coords:
            setattr(self, k, v)

    def assign_coords(self, **kwargs):
        for k, v in kwargs.items():
            setattr(self, k, np.asarray(v))
        return self


reference.xr = types.SimpleNamespace(DataArray=Recorded)
reference.AltimetryResult = lambda res: res
VERTICAL = []
_vertical = reference.NadirSARAltimetry.vertical_scattering_distribution


def recording_vertical(self, *args, **kwargs):
    out = _vertical(self, *args, **kwargs)
    VERTICAL.append((np.array(out[0], float), np.array(out[1], float), np.array(self.t_interface, float)))
    return out


reference.NadirSARAltimetry.vertical_scattering_distribution = recording_vertical


def sensors_of_the_list(module):
    return {"cryosat2_sarm": module.cryosat2_sarm(), "cryosat2_sarm_circular_tilted": module.cryosat2_sarm(0.1, 0.2, True),
            "sentinel3_sarm_Ku_ocean": module.sentinel3_sarm("Ku", "ocean"), "sentinel3_sarm_C_landice": module.sentinel3_sarm("C", "landice"),
            "sentinel3_sarm_C_seaice": module.sentinel3_sarm("C", "seaice"), "cristal_Ku": module.cristal("Ku"),
            "cristal_Ka_circular": module.cristal("Ka", force_circular_antenna=True)}


def sensor_attributes(module):
    out = {}
    for key, one in sensors_of_the_list(module).items():
        out[key] = np.array([float(np.ravel(getattr(one, n))[0]) for n in SENSOR_ATTRIBUTES])
        out[key + ".window_channel"] = np.array([one.doppler_window, list(one.channel_map)[0]])
    out["names"] = np.array(SENSOR_ATTRIBUTES)
    return out


def main():
    np.savez(os.path.join(HERE, "sar_altimeter_list.npz"), **sensor_attributes(sar_altimeter_list))
    for case in CASES:
        del VERTICAL[:]
        sensor, sp = make_sensor(case, API), build_snowpack(case, API)
        options = solver_options(case)
        oversampled = options.get("return_oversampled", False)
        options["return_oversampled"] = True
        with contextlib.redirect_stdout(io.StringIO()):   # (the reference prints from __init__ and from Dinardo18)
            model = make_model("iba", "nadir_sar_altimetry", rtsolver_options=options)
            emmodels = model.prepare_emmodels(sensor, sp)
            solver = model.rtsolver(**options) if isinstance(model.rtsolver, type) else model.rtsolver
            res = solver.solve(sp, emmodels, sensor)
        ddm = np.asarray(res.values, float)[..., 0, 0]
        ddm = ddm if ddm.ndim == 3 else ddm[None]
        names = [str(n) for n in getattr(res, "contribution", [])]
        ost, osd = solver.oversampling_time, solver.oversampling_doppler
        delay, fd, z_gate = np.asarray(res.delay, float), np.asarray(res.doppler_frequency, float), np.asarray(res.z_gate.values, float)
        gate, doppler_bin = np.asarray(res.gate, float), np.asarray(res.doppler_bin, float)
        if not oversampled:   # what coarsen(delay=ost, doppler_frequency=osd).mean() does to the data and to every coordinate
            ddm = ddm.reshape(ddm.shape[0], sensor.ngate, ost, sensor.ndoppler, osd).mean(axis=(2, 4))
            delay, gate = delay.reshape(-1, ost).mean(axis=1), gate.reshape(-1, ost).mean(axis=1)
            fd, doppler_bin = fd.reshape(-1, osd).mean(axis=1), doppler_bin.reshape(-1, osd).mean(axis=1)
            z_gate = z_gate[::ost]   # (the reference's own `self.z_gate[:: self.oversampling_time]`)
        vertical, echo, t_interface = VERTICAL[-1]
        arrays = dict(ddm=ddm, delay=delay, doppler_frequency=fd, gate=gate, doppler_bin=doppler_bin, z_gate=z_gate,
                      vertical=vertical, echo=np.atleast_2d(echo), t_interface=t_interface)
        for name, a in arrays.items():
            finite = np.isfinite(a) | (np.isnan(a) if name == "z_gate" else False)
            assert np.all(finite), (case["name"], name, "not finite")
        if case["name"] == "last_sample":
            shift = np.round(t_interface * sensor.pulse_bandwidth * ost)
            assert shift[1] == sensor.ngate * ost - 1, shift
        np.savez_compressed(os.path.join(HERE, "nadir_sar_altimetry_" + case["name"] + ".npz"), contributions=np.array(names), **arrays)
        print(case["name"], "map", ddm.shape, "peak %.4g" % np.abs(ddm).max(), "sub-gates with volume:", vertical.shape, "echo", echo.shape,
              "shifts", np.round(t_interface * sensor.pulse_bandwidth * ost))


if __name__ == "__main__":
    main()
