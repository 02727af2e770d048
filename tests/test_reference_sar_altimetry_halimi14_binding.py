"""The reference-side binding of the nadir SAR altimetry solver with the Halimi14 delay-Doppler model, EXECUTED (as
tests/test_reference_sar_altimetry_binding.py): the real smrt package (skipped where it is absent) runs its own make_model /
Model.run / concat_results with smrt_amd registered as a plugin package and `delay_doppler_model="halimi14"` -- as a name and as
the reference's own class, which is recognised by its class name -- on its own Snowpack, TerrainInfo and Altimeter objects,
through `runner=HipBatchRunner()` and through `parallel_computation="none"`.  There is no GPU here: `get_context` is routed to
the CPU build of the device source; the numbers are held to the fixtures the reference's own solver made."""
import warnings

import numpy as np
import pytest

from nadir_sar_altimetry_halimi14_restatement import REL_BAR, build_snowpack, case_by_name, make_sensor, model_options, solver_options
from test_nadir_sar_altimetry_halimi14_cpu import TableContext, golden, host_lib  # noqa: F401  (host_lib is a fixture)
from test_reference_altimetry_binding import smrt_ref  # noqa: F401  (a fixture: skips where the reference is absent)
from test_reference_sar_altimetry_binding import reference_api


@pytest.fixture()
def on_host(host_lib, monkeypatch):  # noqa: F811
    from smrt_amd.rtsolver import nadir_sar_altimetry as module

    ctx = TableContext(host_lib)
    monkeypatch.setattr(module, "get_context", lambda device=None: ctx)
    return ctx


@pytest.mark.parametrize("name, as_class", [("widening2", False), ("plrm", True), ("iem_surface", False)])
def test_reference_model_run_through_hip_batch_runner(name, as_class, smrt_ref, on_host):  # noqa: F811
    from smrt.core import plugin
    from smrt.core.plugin import register_package
    from smrt.core.result import AltimetryResult
    from smrt.rtsolver.delay_doppler_model.halimi14 import Halimi14 as ReferenceHalimi14
    from smrt_amd.rtsolver.nadir_sar_altimetry import NadirSARAltimetry
    from smrt_amd.runner.hip_batch_runner import HipBatchRunner

    case, api, g = case_by_name(name), reference_api(smrt_ref), golden(case_by_name(name))
    plugin.user_plugin_package[:] = []          # the reference's own snowpacks, interfaces, substrate, terrain and sensor ...
    sensor = make_sensor(case, api)
    sps = [build_snowpack(case, api) for _ in range(3)]
    assert all(type(o).__module__.startswith("smrt.") for sp in sps for o in sp.interfaces + [sp, sp.terrain_info, sensor])
    register_package("smrt_amd")                # ... and this package's solver behind the reference's make_model
    options = solver_options(case)
    if as_class:
        options["delay_doppler_model"] = ReferenceHalimi14
    m = smrt_ref.make_model("iba", "nadir_sar_altimetry", rtsolver_options=options)
    assert m.rtsolver is NadirSARAltimetry
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")         # (the coherent echo)
        res = m.run(sensor, sps, runner=HipBatchRunner())      # the reference's Model.run and concat_results: one device batch
        one = m.run(sensor, sps[0], parallel_computation="none")
    p = on_host.last_params.struct              # the options are carried over
    assert (p.delay_doppler_model, bool(p.slant_range_correction), p.delay_window_widening) == (1,) + tuple(model_options(case).values())
    assert on_host.calls == 2 and isinstance(res, AltimetryResult) and type(res.data).__module__.split(".")[0] == "xarray"
    names = list(g["contributions"])
    assert res.data.dims == ("snowpack",) + (("contribution",) if names else ()) + ("delay", "doppler_frequency", "theta_inc", "theta")
    values = np.asarray(res.data.values)[..., 0, 0]
    peak = np.abs(g["ddm"][-1]).max()
    for k in range(3):
        w = values[k] if names else values[k][None]
        assert w.shape == g["ddm"].shape and np.abs(w - g["ddm"]).max() <= REL_BAR * peak
    assert isinstance(one, AltimetryResult) and np.array_equal(np.asarray(one.data.values), np.asarray(res.data.values)[0])
    z = np.asarray(one.z_gate.values)
    ok = ~np.isnan(g["z_gate"])
    assert np.array_equal(np.isnan(z), ~ok) and np.abs(z[ok] - g["z_gate"][ok]).max() <= 1e-12 * np.abs(g["z_gate"][ok]).max()
