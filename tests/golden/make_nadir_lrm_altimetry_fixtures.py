#!/usr/bin/env python
"""Fixtures of the nadir LRM altimetry solver.  RUNS ONLY WHERE THE REFERENCE PACKAGE IS (its directory in SMRT_REFERENCE, by
default next to this repository), with the stand-ins of tests/golden/_refstubs for xarray and numba, like
make_multifresnel_fixtures.py.

For every case of tests/nadir_lrm_altimetry_restatement.py:CASES it runs the reference's NadirLRMAltimetry.solve in this process
and stores, as tests/golden/nadir_lrm_altimetry_<name>.npz: the waveform per contribution and the total, delay, gate, z_gate, the
per-layer eps, ke and backward scattering, and the vertical distribution before the convolution; lrm_altimeter_list.npz holds every
attribute of every channel of the reference's altimeter list.  The stand-in xarray lacks assign_coords, so `xr` and
`AltimetryResult` are replaced IN THE NAMESPACE OF THE REFERENCE MODULE by a recorder; nothing of the reference is changed on disk.

The script FAILS if the reference raises on a case, if a value is not finite (z_gate below the snowpack is NaN by design), or if
the reference's merged depth grid did not obey the tie rule the restatement and the device define: at equal depth a layer
boundary precedes a gate.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_nadir_lrm_altimetry_fixtures.py
"""
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
from smrt.inputs import lrm_altimeter_list  # noqa: E402
from smrt.rtsolver import nadir_lrm_altimetry as reference  # noqa: E402

from nadir_lrm_altimetry_restatement import CASES, build_snowpack, make_sensor, solver_options  # noqa: E402

API = types.SimpleNamespace(make_snowpack=make_snowpack, make_soil=make_soil, make_interface=make_interface,
                            lrm_altimeter_list=lrm_altimeter_list)


class Recorded:
    """What the reference builds its result from: values, coordinates, the gate coordinate, z_gate."""

    def __init__(self, values, coords=None):
        self.values = np.asarray(values)
        self.coords = [(c[0], np.asarray(c[1])) for c in coords if isinstance(c, tuple)]   # (z_gate is given a bare array)
        for k, v in self.coords:
            setattr(self, k, v)

    def assign_coords(self, **kwargs):
        for k, v in kwargs.items():
            setattr(self, k, np.asarray(v))
        return self


reference.xr = types.SimpleNamespace(DataArray=Recorded)
reference.AltimetryResult = lambda res: res
GRIDS, VERTICAL = [], []
_grid = reference.NadirLRMAltimetry.combined_depth_grid
_vertical = reference.NadirLRMAltimetry.vertical_scattering_distribution


def recording_grid(self):
    out = _grid(self)
    GRIDS.append((np.array(out[0]), np.array(out[4]), np.array(self.snowpack.z), np.array(self.z_gate)))
    return out


def recording_vertical(self, *args, **kwargs):
    out = _vertical(self, *args, **kwargs)
    VERTICAL.append(np.atleast_2d(np.array(out)))
    return out


reference.NadirLRMAltimetry.combined_depth_grid = recording_grid
reference.NadirLRMAltimetry.vertical_scattering_distribution = recording_vertical


def tie_rule_obeyed(z_top, b_interface, z_lay, z_gate):
    """Wherever a boundary and a gate have the same depth, the boundary comes first in the reference's sorted grid."""
    z = np.concatenate([z_top, [np.inf]])
    for p in range(len(b_interface) - 1):
        if z[p] == z[p + 1] and not b_interface[p] and b_interface[p + 1]:
            return False
    return bool(b_interface[0])


def sensor_attributes():
    out = {}
    sensors = {"envisat_ra2": lrm_altimeter_list.envisat_ra2(), "sentinel3_sral": lrm_altimeter_list.sentinel3_sral(),
               "saral_altika": lrm_altimeter_list.saral_altika(), "cryosat2_lrm": lrm_altimeter_list.cryosat2_lrm(),
               "asiras_lam": lrm_altimeter_list.asiras_lam(altitude=1000.0),
               "envisat_ra2_tilted": lrm_altimeter_list.envisat_ra2("Ku", pitch_angle_deg=0.1, roll_angle_deg=0.2)}
    names = ("frequency", "altitude", "pulse_bandwidth", "beamwidth_alongtrack", "beamwidth_acrosstrack", "antenna_gain", "ngate",
             "ndoppler", "nominal_gate", "pitch_angle", "roll_angle", "off_nadir_angle", "alpha", "pulse_repetition_frequency",
             "velocity", "wavelength", "theta_inc_deg", "theta_deg", "phi_deg")
    for key, s in sensors.items():
        for one in (s.sensor_list if hasattr(s, "sensor_list") else [s]):
            channel = list(one.channel_map)[0]
            out[f"{key}.{channel}"] = np.array([float(np.ravel(getattr(one, n))[0]) for n in names])
    out["names"] = np.array(names)
    return out


def main():
    np.savez(os.path.join(HERE, "lrm_altimeter_list.npz"), **sensor_attributes())
    for case in CASES:
        del GRIDS[:], VERTICAL[:]
        sensor, sp = make_sensor(case, API), build_snowpack(case, API)
        model = make_model(case.get("emmodel", "iba"), "nadir_lrm_altimetry", rtsolver_options=solver_options(case))
        emmodels = model.prepare_emmodels(sensor, sp)
        solver = model.rtsolver(**solver_options(case)) if isinstance(model.rtsolver, type) else model.rtsolver
        res = solver.solve(sp, emmodels, sensor)
        w = np.asarray(res.values, float)[..., 0, 0]
        w = w if w.ndim == 2 else w[None]
        eps = np.array([em.effective_permittivity().real for em in emmodels])
        ke = np.array([float(np.mean(em.ke(mu=[1.0]).diagonal)) for em in emmodels])
        bs = np.array([float(np.real(np.squeeze(em.phase(mu_s=-1.0, mu_i=1.0, dphi=np.pi, npol=2)[0, 0]))) / (4 * np.pi)
                       for em in emmodels]) / eps
        arrays = dict(waveform=w, delay=np.asarray(res.delay, float), gate=np.asarray(res.gate, float),
                      z_gate=np.asarray(res.z_gate.values, float), eps=eps, ke=ke, backward_scattering=bs, vertical=VERTICAL[-1])
        for name, a in arrays.items():
            finite = np.isfinite(a) | (np.isnan(a) if name == "z_gate" else False)
            assert np.all(finite), (case["name"], name, "not finite")
        assert GRIDS and all(tie_rule_obeyed(*g) for g in GRIDS), (case["name"], "a gate precedes a boundary of the same depth")
        np.savez(os.path.join(HERE, "nadir_lrm_altimetry_" + case["name"] + ".npz"), **arrays)
        print(case["name"], "waveform", w.shape, "peak %.4g" % np.abs(w).max(), "vertical", VERTICAL[-1].shape,
              "gates in the snowpack:", int(np.isfinite(arrays["z_gate"]).sum()))


if __name__ == "__main__":
    main()
