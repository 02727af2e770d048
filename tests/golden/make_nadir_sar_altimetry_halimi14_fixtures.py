#!/usr/bin/env python
"""Fixtures of the nadir SAR altimetry solver with the delay-Doppler model of Halimi et al. 2014.  RUNS ONLY WHERE THE REFERENCE
PACKAGE IS (its directory in SMRT_REFERENCE, by default next to this repository), with the stand-ins of tests/golden/_refstubs for
xarray and numba, like make_nadir_sar_altimetry_fixtures.py.

For every case of tests/nadir_sar_altimetry_halimi14_restatement.py:CASES it runs the reference's NadirSARAltimetry.solve in this
process with return_oversampled=True (the stand-in xarray has no coarsen) and stores as
tests/golden/nadir_sar_altimetry_halimi14_<name>.npz what the Dinardo18 fixtures hold, and: `table`, the reference's own
Halimi14.delay_doppler_map (where it has at most TABLE_STORED_UP_TO samples), `last_column`, the last Doppler column of the
impulse response it hands to its convolutions, `compensation`, the rows every column is moved up.

`xr` and `AltimetryResult` are replaced IN THE NAMESPACE OF THE REFERENCE'S SOLVER MODULE by a recorder.  The stand-in numba runs
_jit_delay_compensation as plain Python, where numpy.floor gives a float that cannot slice: `np` is replaced IN THE NAMESPACE OF
THE REFERENCE'S delay_doppler_utils MODULE by a proxy that forwards everything and whose floor returns an int.  Nothing of the
reference is changed on disk.

The script FAILS if the reference raises on a case, if a value is not finite (z_gate below the snowpack is NaN by design), or if a
case does not show what it is there for.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_nadir_sar_altimetry_halimi14_fixtures.py
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
from smrt.rtsolver.delay_doppler_model import delay_doppler_utils, halimi14  # noqa: E402

from make_nadir_sar_altimetry_fixtures import Recorded  # noqa: E402  (it replaces xr and AltimetryResult, and records the vertical part)
from make_nadir_sar_altimetry_fixtures import VERTICAL  # noqa: E402
from nadir_sar_altimetry_halimi14_restatement import (CASES, TABLE_STORED_UP_TO, build_snowpack, make_sensor, model_options,  # noqa: E402
                                                      solver_options)

API = types.SimpleNamespace(make_snowpack=make_snowpack, make_soil=make_soil, make_interface=make_interface,
                            sar_altimeter_list=sar_altimeter_list, TerrainInfo=TerrainInfo)
assert reference.xr.DataArray is Recorded


class NumpyWithIntegerFloor:
    """numpy, but floor returns a Python int (what the slice of _jit_delay_compensation needs without numba)."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def floor(x):
        return int(np.floor(x))


delay_doppler_utils.np = NumpyWithIntegerFloor()
RECORDED = {}
_convolution, _map = halimi14.numerical_convolution, halimi14.Halimi14.delay_doppler_map


def recording_convolution(fsir, *args, **kwargs):
    RECORDED["fsir"] = np.array(fsir, float)
    return _convolution(fsir, *args, **kwargs)


def recording_map(self, terrain_info):
    RECORDED["table"] = np.array(_map(self, terrain_info), float)
    return RECORDED["table"]


halimi14.numerical_convolution = recording_convolution
halimi14.Halimi14.delay_doppler_map = recording_map


def main():
    for case in CASES:
        del VERTICAL[:]
        RECORDED.clear()
        sensor, sp = make_sensor(case, API), build_snowpack(case, API)
        options = solver_options(case)
        oversampled = options.get("return_oversampled", False)
        options["return_oversampled"] = True
        with contextlib.redirect_stdout(io.StringIO()):   # (the reference prints from __init__)
            model = make_model("iba", "nadir_sar_altimetry", rtsolver_options=options)
            emmodels = model.prepare_emmodels(sensor, sp)
            solver = model.rtsolver(**options) if isinstance(model.rtsolver, type) else model.rtsolver
            res = solver.solve(sp, emmodels, sensor)
        assert type(solver.delay_doppler_model).__name__ == "Halimi14"
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
            z_gate = z_gate[::ost]
        vertical, echo, t_interface = VERTICAL[-1]
        fsir, table = RECORDED["fsir"], RECORDED["table"]
        N, Nb, widening = sensor.ngate * ost, sensor.ndoppler * osd, model_options(case)["delay_window_widening"]
        assert fsir.shape == (N * widening, Nb) and table.shape == (N, Nb)
        idelta_r1 = delay_doppler_utils._compute_idelta_r1(sensor, ost, osd, True)
        compensation = np.floor(idelta_r1 * (np.arange(Nb) - Nb // 2 + 0.5) ** 2)
        arrays = dict(ddm=ddm, delay=delay, doppler_frequency=fd, gate=gate, doppler_bin=doppler_bin, z_gate=z_gate,
                      vertical=vertical, echo=np.atleast_2d(echo), t_interface=t_interface, last_column=fsir[:, -1], compensation=compensation)
        if table.size <= TABLE_STORED_UP_TO:
            arrays["table"] = table
        for name, a in arrays.items():
            finite = np.isfinite(a) | (np.isnan(a) if name == "z_gate" else False)
            assert np.all(finite), (case["name"], name, "not finite")
        # what the cases are there for
        name = case["name"]
        shift = np.round(t_interface * sensor.pulse_bandwidth * ost)
        assert np.abs(table).max() > 0 and np.abs(ddm[-1]).max() > 0, name
        if name == "last_sample":
            assert shift[1] == N - 1, shift
        if name == "shifted_out":
            assert compensation.max() >= N * widening and np.all(table[:, compensation >= N * widening] == 0), compensation
            assert np.any(table[:, compensation < N] != 0)
        if name == "last_column":
            assert fsir[:, -1].min() < 0, fsir[:, -1]
        if name == "plrm":
            assert np.all(np.abs(table).max(axis=0) > 0)      # no column is moved out
        if name == "narrow_pdf":
            assert 2 * case["sigma_surface"] / 299792458.0 < 1 / (ost * sensor.pulse_bandwidth)
        if name == "n63_d60":
            assert N % 2 == 1 and Nb % 64
        if name == "iem_surface":
            assert not any(hasattr(i, "mean_square_slope") for i in sp.interfaces) and np.atleast_2d(echo)[1, 0] > 0
        np.savez_compressed(os.path.join(HERE, "nadir_sar_altimetry_halimi14_" + name + ".npz"), contributions=np.array(names), **arrays)
        print(name, "map", ddm.shape, "peak %.4g" % np.abs(ddm).max(), "table", table.shape, "largest compensation", compensation.max(),
              "most negative last column %.3g" % fsir[:, -1].min(), "shifts", shift)


if __name__ == "__main__":
    main()
