"""The reference-side binding of the nadir SAR altimetry solver, EXECUTED (style of tests/test_reference_altimetry_binding.py):
the real smrt package (skipped where it is absent) runs its own make_model / Model.run / concat_results with smrt_amd registered
as a plugin package, on its own Snowpack, TerrainInfo and Altimeter objects, through `runner=HipBatchRunner()` and through
`parallel_computation="none"`.  There is no GPU here: `get_context` is routed to the CPU build of the device source, so the
numbers are the kernels' own; they are held to the fixtures the reference's own solver made."""
import types

import numpy as np
import pytest

from nadir_sar_altimetry_restatement import REL_BAR, build_snowpack, case_by_name, make_sensor, solver_options
from test_nadir_sar_altimetry_cpu import HostContext, golden, host_lib  # noqa: F401  (host_lib is a fixture)
from test_reference_altimetry_binding import smrt_ref  # noqa: F401  (a fixture: skips where the reference is absent)


@pytest.fixture()
def on_host(host_lib, monkeypatch):  # noqa: F811
    from smrt_amd.rtsolver import nadir_sar_altimetry as module

    ctx = HostContext(host_lib)
    monkeypatch.setattr(module, "get_context", lambda device=None: ctx)
    return ctx


def reference_api(smrt):
    from smrt.core.terrain import TerrainInfo
    from smrt.inputs import sar_altimeter_list

    return types.SimpleNamespace(make_snowpack=smrt.make_snowpack, make_soil=smrt.make_soil, make_interface=smrt.make_interface,
                                 sar_altimeter_list=sar_altimeter_list, TerrainInfo=TerrainInfo)


@pytest.mark.parametrize("name", ["reduced_L1", "n64_d64_basic_coherent", "deep_pruned"])
def test_reference_model_run_through_hip_batch_runner(name, smrt_ref, on_host):  # noqa: F811
    from smrt.core import plugin
    from smrt.core.plugin import register_package
    from smrt.core.result import AltimetryResult
    from smrt_amd.rtsolver.nadir_sar_altimetry import NadirSARAltimetry
    from smrt_amd.runner.hip_batch_runner import HipBatchRunner

    case, api, g = case_by_name(name), reference_api(smrt_ref), golden(case_by_name(name))
    plugin.user_plugin_package[:] = []          # the reference's own snowpacks, interfaces, substrate, terrain and sensor ...
    sensor = make_sensor(case, api)
    sps = [build_snowpack(case, api) for _ in range(3)]
    assert all(type(o).__module__.startswith("smrt.") for sp in sps for o in sp.interfaces + [sp, sp.terrain_info, sensor])
    register_package("smrt_amd")                # ... and this package's solver behind the reference's make_model
    m = smrt_ref.make_model("iba", "nadir_sar_altimetry", rtsolver_options=solver_options(case))
    assert m.rtsolver is NadirSARAltimetry
    res = m.run(sensor, sps, runner=HipBatchRunner())      # the reference's Model.run and concat_results: one device batch
    assert on_host.calls == 1 and isinstance(res, AltimetryResult) and type(res.data).__module__.split(".")[0] == "xarray"
    names = list(g["contributions"])
    assert res.data.dims == ("snowpack",) + (("contribution",) if names else ()) + ("delay", "doppler_frequency", "theta_inc", "theta")
    values = np.asarray(res.data.values)[..., 0, 0]
    peak = np.abs(g["ddm"][-1]).max()
    for k in range(3):
        w = values[k] if names else values[k][None]
        assert w.shape == g["ddm"].shape and np.abs(w - g["ddm"]).max() <= REL_BAR * peak
    # the rtsolver protocol: one solve per simulation, the reference's own result with z_gate as the reference sets it
    one = m.run(sensor, sps[0], parallel_computation="none")
    assert isinstance(one, AltimetryResult) and np.array_equal(np.asarray(one.data.values), np.asarray(res.data.values)[0])
    z = np.asarray(one.z_gate.values)
    ok = ~np.isnan(g["z_gate"])
    assert np.array_equal(np.isnan(z), ~ok) and np.abs(z[ok] - g["z_gate"][ok]).max() <= 1e-12 * np.abs(g["z_gate"][ok]).max()
    assert all(sp.terrain_info.sigma_surface == case["sigma_surface"] for sp in sps)
