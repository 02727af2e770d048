"""The reference-side binding of the nadir LRM altimetry solver, EXECUTED (style of tests/test_reference_binding.py): the real
smrt package (skipped where it is absent) runs its own make_model / Model.run / concat_results with smrt_amd registered as a
plugin package, on its own Snowpack and Altimeter objects, through `runner=HipBatchRunner()` and through
`parallel_computation="none"` (one solve per simulation).  There is no GPU here: `get_context` is routed to the CPU build of the
device source, so the numbers are the kernels' own; they are held to the fixtures the reference's own solver made."""
import os
import sys
import types

import numpy as np
import pytest

from conftest import ROOT
from nadir_lrm_altimetry_restatement import REL_BAR, build_snowpack, case_by_name, make_sensor, solver_options
from test_nadir_lrm_altimetry_cpu import HostContext, golden, host_lib  # noqa: F401  (host_lib is a fixture)

REFERENCE = "/root/reference"
STUBS = os.path.join(ROOT, "tests", "golden", "_refstubs")


@pytest.fixture(scope="module")
def smrt_ref():
    if not os.path.isdir(os.path.join(REFERENCE, "smrt")):
        pytest.skip("the reference package is only present in the build container")
    sys.dont_write_bytecode = True
    added = [p for p in (STUBS, REFERENCE) if p not in sys.path]
    sys.path[:0] = added
    import smrt
    from smrt.core import plugin

    before = list(plugin.user_plugin_package)
    yield smrt
    plugin.user_plugin_package[:] = before
    for p in added:
        sys.path.remove(p)


@pytest.fixture()
def on_host(host_lib, monkeypatch):  # noqa: F811
    from smrt_amd.rtsolver import nadir_lrm_altimetry as module

    ctx = HostContext(host_lib)
    monkeypatch.setattr(module, "get_context", lambda device=None: ctx)
    return ctx


def reference_api(smrt):
    from smrt.inputs import lrm_altimeter_list

    return types.SimpleNamespace(make_snowpack=smrt.make_snowpack, make_soil=smrt.make_soil, make_interface=smrt.make_interface,
                                 lrm_altimeter_list=lrm_altimeter_list)


@pytest.mark.parametrize("name", ["flat_L3_contrib", "rough_tis4", "rough_fast_coherent_sigma"])
def test_reference_model_run_through_hip_batch_runner(name, smrt_ref, on_host):
    from smrt.core.plugin import register_package
    from smrt.core.result import AltimetryResult
    from smrt_amd.rtsolver.nadir_lrm_altimetry import NadirLRMAltimetry
    from smrt_amd.runner.hip_batch_runner import HipBatchRunner

    from smrt.core import plugin

    case, api, g = case_by_name(name), reference_api(smrt_ref), golden(case_by_name(name))
    plugin.user_plugin_package[:] = []          # the reference's own snowpacks, interfaces, substrate and sensor ...
    sensor = make_sensor(case, api)
    sps = [build_snowpack(case, api) for _ in range(3)]
    assert all(type(o).__module__.startswith("smrt.") for sp in sps for o in sp.interfaces + [sp, sensor])
    register_package("smrt_amd")                # ... and this package's solver behind the reference's make_model
    m = smrt_ref.make_model("iba", "nadir_lrm_altimetry", rtsolver_options=solver_options(case))
    assert m.rtsolver is NadirLRMAltimetry
    res = m.run(sensor, sps, runner=HipBatchRunner())      # the reference's Model.run and concat_results: one device batch
    assert on_host.calls == 1 and isinstance(res, AltimetryResult) and type(res.data).__module__.split(".")[0] == "xarray"
    contributions = solver_options(case).get("return_contributions", False)
    assert res.data.dims == ("snowpack",) + (("contribution",) if contributions else ()) + ("delay", "theta_inc", "theta")
    values = np.asarray(res.data.values)[..., 0, 0]
    peak = np.abs(g["waveform"][-1]).max()
    for k in range(3):
        w = values[k] if contributions else values[k][None]
        assert np.abs(w - g["waveform"]).max() <= REL_BAR * peak
    # the rtsolver protocol: one solve per simulation, the reference's own result with z_gate as the reference sets it
    one = m.run(sensor, sps[0], parallel_computation="none")
    assert isinstance(one, AltimetryResult) and np.array_equal(np.asarray(one.data.values), np.asarray(res.data.values)[0])
    z = np.asarray(one.z_gate.values)
    ok = ~np.isnan(g["z_gate"])
    assert np.array_equal(np.isnan(z), ~ok) and np.abs(z[ok] - g["z_gate"][ok]).max() <= 1e-12 * np.abs(g["z_gate"][ok]).max()
    assert np.abs(np.asarray(one.data.coords[-3][1] if isinstance(one.data.coords, list) else one.data.coords["delay"]) - g["delay"]).max() \
        <= 1e-12 * np.abs(g["delay"]).max()
    # surface attributes of the reference's snowpack travel with it
    assert all(getattr(sp, a, 0) == case.get(a, 0) for sp in sps for a in ("sigma_surface", "surface_slope"))
