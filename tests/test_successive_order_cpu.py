"""The successive-order solver without a GPU: the NumPy restatement against every fixture, the DEVICE arithmetic
(smrt_amd/csrc/successive_order_kernel.hpp) compiled with g++ against every fixture and against the restatement on the
substrate cases, the substrate emission against the DORT oracle, and the Python layer (plugin, options, result labels,
refusals, error handling) driven end to end with the CPU build of the kernels in place of the GPU context.

Tolerances: restatement against fixtures 1e-9 K (two float64 implementations of the same sums differ by ~1e-12 K; the
package's bar of 1e-6 K keeps its margin for the device); device source against fixtures / restatement 1e-6 K (the
project's bar for a brightness temperature); layer scalars: eps 1e-12, ks 1e-11, ka 1e-10 relative (tests/test_gpu_parity.py)."""
import ctypes as C
import os
import sys
import threading
import types

import numpy as np
import pytest

import smrt_amd
from host_build import host_library
from smrt_amd import _native, make_model, sensor_list
from smrt_amd.core.error import SMRTError
from smrt_amd.inputs.make_medium import make_interface, make_snowpack, make_soil
from successive_order_restatement import (CASES, FIXTURE_CASES, SUBSTRATE_CASES, TB_ATOL, build_snowpack, case_by_name,
                                          solve_case, solver_options)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def api():
    from smrt_amd.substrate.reflector import make_reflector

    return types.SimpleNamespace(make_snowpack=make_snowpack, make_soil=make_soil, make_reflector=make_reflector)


def golden(case):
    return np.load(os.path.join(GOLDEN, "successive_order_" + case["name"] + ".npz"))


_RESTATED = {}


def restated(case):
    """The restatement of a case, computed once and shared (never modified)."""
    if case["name"] not in _RESTATED:
        _RESTATED[case["name"]] = solve_case(case)
    return _RESTATED[case["name"]]


def assert_matches(values, reference, atol, what):
    """values, reference [2, n_theta, orders + 1] kelvin; exact zeros exactly where the reference has them."""
    err = float(np.abs(values - reference).max())
    print(f"{what}: largest difference {err:.3e} K (bar {atol:g})")
    assert np.array_equal(values == 0.0, reference == 0.0), what
    assert err <= atol, (what, err)
    return err


# ---- restatement against the fixtures -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FIXTURE_CASES, ids=lambda c: c["name"])
def test_restatement_reproduces_the_fixture(case):
    g = golden(case)
    sol, layers = restated(case)
    assert_matches(sol["tb"], g["tb"], 1e-9, "restatement " + case["name"])
    assert sol["orders"] == len(g["max_radiance"])
    assert np.array_equal(sol["sublayers"], g["sublayers"]) and np.array_equal(sol["streams"], g["streams"])
    assert np.abs(sol["max_radiance"] / g["max_radiance"] - 1.0).max() < 1e-12


def test_fixtures_cover_what_they_must():
    gs = {c["name"]: golden(c) for c in FIXTURE_CASES}
    cap = {c["name"]: c["n_iteration_max"] for c in FIXTURE_CASES}
    assert any(len(g["max_radiance"]) < cap[n] for n, g in gs.items()) and any(len(g["max_radiance"]) == cap[n] for n, g in gs.items())
    assert any(len(set(g["streams"])) > 1 for g in gs.values())
    assert any(g["sublayers"].min() == 1 for g in gs.values()) and any(g["sublayers"].max() > 16 for g in gs.values())
    g = gs["iba_L1_n4"]   # stops by tolerance after 9 orders; the rest are exact zeros
    assert len(g["max_radiance"]) == 9 and np.all(g["tb"][:, :, 9:12] == 0.0) and np.all(g["tb"][:, :, :9] > 0.0)
    assert gs["iba_L20_n32"]["streams"].max() == 32


# ---- the device source on the CPU ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_lib():
    lib = host_library("libsmrt_successive_order_host.so", "successive_order_host.cpp")
    lib.smrt_successive_order_host_run.restype = C.c_int32
    return lib


def host_run(lib, batch, n_iteration_max, relative_tolerance, order=0):
    o = _native.SuccessiveOrderOutput(batch, batch.n_pairs, n_iteration_max)
    rc = lib.smrt_successive_order_host_run(C.byref(batch.struct), C.c_int32(n_iteration_max), C.c_double(relative_tolerance),
                                            C.c_int32(order), *o.pointers())
    assert rc == 0
    return o


def pack_case(case):
    """The PackedBatch of a case through the solver's own packer (DORT's packing)."""
    from smrt_amd.rtsolver.successive_order import SuccessiveOrder

    solver = SuccessiveOrder(**solver_options(case))
    sp = build_snowpack(case, api())
    sensor = sensor_list.passive(case["frequency"], case["theta"])
    return solver._packer()._pack(sensor, [sp], np.array([case["frequency"]]), case["emmodel"]), solver


def assert_layers(out, g, L):
    lay = out.layers[0][:L]
    eps = lay[:, 0] + 1j * lay[:, 1]
    assert np.abs(eps - g["eps"]).max() <= 1e-12 * np.abs(g["eps"]).max()
    assert np.all(np.abs(lay[:, 2] - g["ks"]) <= 1e-11 * np.abs(g["ks"]))
    assert np.all(np.abs(lay[:, 3] - g["ka"]) <= 1e-10 * np.abs(g["ka"]))
    assert np.array_equal(lay[:, 4].astype(int), g["streams"]) and np.array_equal(out.sublayers[0][:L], g["sublayers"])


@pytest.mark.parametrize("case", FIXTURE_CASES, ids=lambda c: c["name"])
def test_device_source_on_the_cpu_reproduces_the_fixture(host_lib, case):
    g = golden(case)
    batch, solver = pack_case(case)
    out = host_run(host_lib, batch, solver.n_iteration_max, solver.relative_tolerance)
    assert out.status[0] == 0 and out.orders[0] == len(g["max_radiance"])
    assert_matches(out.values[0], g["tb"], TB_ATOL, "device source on the CPU " + case["name"])
    assert_layers(out, g, len(case["thickness"]))
    n = out.orders[0]
    assert np.abs(out.max_radiance[0][:n] / g["max_radiance"] - 1.0).max() < 1e-10 and np.all(out.max_radiance[0][n:] == 0.0)


@pytest.mark.parametrize("case", SUBSTRATE_CASES, ids=lambda c: c["name"])
def test_device_source_on_the_cpu_reproduces_the_restatement_on_substrates(host_lib, case):
    sol, _ = restated(case)
    batch, solver = pack_case(case)
    out = host_run(host_lib, batch, solver.n_iteration_max, solver.relative_tolerance)
    assert out.status[0] == 0 and out.orders[0] == sol["orders"]
    assert_matches(out.values[0], sol["tb"], TB_ATOL, "device source on the CPU " + case["name"])


def test_device_source_has_no_race_between_its_phases(host_lib):
    """Fibers visited forwards, backwards and strided give the same bits: no barrier is missing in the sweep kernel."""
    case = case_by_name("iba_refraction_L3_n6")
    batch, solver = pack_case(case)
    outs = [host_run(host_lib, batch, solver.n_iteration_max, solver.relative_tolerance, order) for order in (0, 1, 2)]
    assert np.array_equal(outs[0].raw, outs[1].raw) and np.array_equal(outs[0].raw, outs[2].raw)


# ---- difference 1: the substrate's own emission --------------------------------------------------------------------------
def test_substrate_emission_against_dort():
    """iba_soil_L2_n8 with 30 orders: the total within 0.5 K of the DORT oracle at the same stream count -- twice the largest
    gap seen between the reference's own successive-order total and its DORT on deep snowpacks without substrate (0.05 to
    0.26 K at 8 to 16 streams).  Without the emission term the gap is above 200 K.  (Measured: profiles/successive_order_parity.txt.)"""
    from oracle import dort_oracle as O
    from successive_order_restatement import oracle_snowpack, oracle_substrate, successive_order

    case = case_by_name("iba_soil_L2_n8")
    sol, layers = solve_case(case, n_iteration_max=30)
    dort = O.solve(oracle_snowpack(case), case["frequency"], case["theta"], n_max_stream=case["n_max_stream"],
                   substrate=oracle_substrate(case))
    gap = np.abs(sol["tb"][:, :, -1] - dort)
    cold = successive_order(layers, case["thickness"], case["temperature"], case["frequency"], case["theta"], n_max_stream=8,
                            n_iteration_max=30, substrate=dict(oracle_substrate(case), temperature=0.0))
    gap_cold = np.abs(cold["tb"][:, :, -1] - dort)
    print(f"successive order (30 orders) - DORT oracle on iba_soil_L2_n8: V {gap[0, 0]:.4f} K, H {gap[1, 0]:.4f} K; "
          f"without the substrate's emission: V {gap_cold[0, 0]:.2f} K, H {gap_cold[1, 0]:.2f} K")
    assert gap.max() < 0.5
    assert gap_cold.min() > 100.0


# ---- the Python layer, end to end on the CPU build of the kernels ---------------------------------------------------------
class HostContext:
    """Stands in for DortContext: the same call, answered by the CPU build of the device source."""

    def __init__(self, lib):
        self.lib, self.lock, self.calls = lib, threading.RLock(), 0

    def successive_order_run(self, batch, n_iteration_max=50, relative_tolerance=0.001, pairs=None, workspace_budget=None):
        self.calls += 1
        o = host_run(self.lib, batch, n_iteration_max, relative_tolerance)
        if pairs is not None:
            for name in ("raw", "status", "layers", "streams", "sublayers", "max_radiance", "orders"):
                setattr(o, name, getattr(o, name)[np.asarray(pairs)])
        return o

    def successive_order_launch_info(self):
        return dict(chunks=1, reserved_bytes=0, over_budget=0, budget=0)


@pytest.fixture()
def on_host(host_lib, monkeypatch):
    from smrt_amd.rtsolver import successive_order as module

    ctx = HostContext(host_lib)
    monkeypatch.setattr(module, "get_context", lambda device=None: ctx)
    return ctx


def test_plugin_resolution_and_options():
    from smrt_amd.core.model import make_rtsolver
    from smrt_amd.core.plugin import import_class
    from smrt_amd.rtsolver.successive_order import SuccessiveOrder

    assert import_class("rtsolver", "successive_order") is SuccessiveOrder
    m = make_model("iba", "successive_order", rtsolver_options={"n_max_stream": 8, "n_iteration_max": 12, "error_handling": "nan"})
    solver = m.make_rtsolver_instance()
    assert isinstance(solver, SuccessiveOrder) and solver.n_max_stream == 8 and solver.n_iteration_max == 12
    assert issubclass(make_rtsolver("successive_order", n_iteration_max=3), SuccessiveOrder)
    d = SuccessiveOrder()
    assert (d.n_max_stream, d.n_iteration_max, d.relative_tolerance, d.m_max, d.stream_mode) == (32, 50, 0.001, 2, "most_refringent")
    assert not d.phase_symmetrization and not d.process_coherent_layers and not d.rayleigh_jeans_approximation
    assert d.error_handling == "exception" and d.devices is None
    for bad in (dict(phase_symmetrization=True), dict(process_coherent_layers=True), dict(error_handling="ignore"),
                dict(stream_mode="uniform_air"), dict(n_max_stream=1), dict(n_max_stream=65), dict(n_iteration_max=0),
                dict(relative_tolerance=-1.0), dict(incident_polarizations="H")):
        with pytest.raises(SMRTError):
            SuccessiveOrder(**bad)
    assert [a for a, _ in m.split_axes(sensor_list.passive([19e9, 37e9], [40, 55]))] == ["frequency"]


def test_readme_example_prints_the_fixture(on_host):
    case = case_by_name("iba_tol0_n8")
    sp = build_snowpack(case, api())
    m = make_model("iba", "successive_order", rtsolver_options={"n_max_stream": 8, "n_iteration_max": 12, "relative_tolerance": 0.0})
    res = m.run(sensor_list.passive(37e9, 55), sp)
    g = golden(case)["tb"]
    assert res.data.dims == ("polarization", "theta", "order")
    assert list(res.data.coords["order"]) == list(range(12)) + ["total"]
    assert list(res.data.coords["polarization"]) == ["V", "H"] and np.allclose(res.data.coords["theta"], [55.0])
    assert abs(float(res.TbV(order="total")) - g[0, 0, -1]) < TB_ATOL and abs(float(res.TbV(order=0)) - g[0, 0, 0]) < TB_ATOL
    assert abs(float(res.TbH(order=1)) - g[1, 0, 1]) < TB_ATOL
    other = res.other_data
    assert set(other) >= {"stream_angles", "effective_permittivity", "ks", "ka", "ke", "thickness"}
    assert np.allclose(other["thickness"].values, case["thickness"]) and other["ks"].values.shape == (2,)
    assert np.allclose(other["ke"].values, other["ks"].values + other["ka"].values)
    assert len(other["stream_angles"].values) == 4 and np.all(np.diff(other["stream_angles"].values) > 0)


def test_model_run_batches_into_one_launch_per_group(on_host):
    soil = make_soil("flat", complex(3.0, 0.1), 265.0)
    sps = [make_snowpack([0.2, 0.4 + 0.1 * k], "exponential", density=[250.0, 350.0], temperature=[255.0, 262.0],
                         corr_length=[1e-4, 2e-4], substrate=soil if k % 2 else None) for k in range(4)]
    m = make_model("iba", "successive_order", rtsolver_options={"n_max_stream": 4, "n_iteration_max": 3})
    solver_cls = m.rtsolver
    res = m.run(sensor_list.passive([19e9, 37e9], 53), sps)
    assert on_host.calls == 2          # with and without substrate
    assert res.data.dims == ("frequency", "snowpack", "polarization", "theta", "order") and res.data.shape == (2, 4, 2, 1, 4)
    single = m.run(sensor_list.passive(37e9, 53), sps[1])
    assert np.array_equal(single.data.values, res.data.values[1, 1])
    assert solver_cls is m.rtsolver


def test_out_of_scope_inputs_raise(on_host):
    from smrt_amd.atmosphere.simple_isotropic_atmosphere import SimpleIsotropicAtmosphere
    from smrt_amd.rtsolver.successive_order import SuccessiveOrder
    from smrt_amd.substrate.transparent import Transparent

    kw = dict(density=[300.0], temperature=[260.0], corr_length=[2e-4])
    sp = make_snowpack([1.0], "exponential", **kw)
    m = make_model("iba", "successive_order", rtsolver_options={"n_max_stream": 4, "n_iteration_max": 2})
    with pytest.raises(SMRTError, match="active sensors"):
        m.run(sensor_list.active(13e9, 30), sp)
    atmosphere = SimpleIsotropicAtmosphere(tb_down=20.0, tb_up=18.0, transmittance=0.9)
    with pytest.raises(SMRTError, match="the successive_order solver can not handle atmosphere yet."):
        m.run(sensor_list.passive(37e9, 55), atmosphere + sp)
    with pytest.raises(SMRTError, match="the successive_order solver can not handle atmosphere yet."):
        SuccessiveOrder().solve(sp, [None], sensor_list.passive(37e9, 55), atmosphere=atmosphere)
    rough = make_snowpack([1.0], "exponential", interface=[make_interface("geometrical_optics_backscatter", mean_square_slope=0.03)], **kw)
    with pytest.raises(SMRTError, match="rough interfaces"):
        m.run(sensor_list.passive(37e9, 55), rough)
    rough_soil = make_snowpack([1.0], "exponential", substrate=make_soil("geometrical_optics_backscatter", complex(8.0, 1.0), 268.0,
                                                                        mean_square_slope=0.05), **kw)
    with pytest.raises(SMRTError, match="substrate"):
        m.run(sensor_list.passive(37e9, 55), rough_soil)
    with pytest.raises(SMRTError, match="evaluated on the host"):
        make_model("rayleigh", "successive_order", rtsolver_options={"n_max_stream": 4}).run(
            sensor_list.passive(37e9, 55), make_snowpack([1.0], "sticky_hard_spheres", density=[300.0], temperature=[260.0], radius=[2e-4],
                                                         stickiness=[0.2]))
    with pytest.raises(SMRTError, match="process_coherent_layers"):
        make_model("iba", "successive_order", rtsolver_options={"process_coherent_layers": True}).run(sensor_list.passive(37e9, 55), sp)
    # a transparent substrate is no substrate
    clear = make_snowpack([1.0], "exponential", substrate=Transparent(), **kw)
    a, b = m.run(sensor_list.passive(37e9, 55), clear), m.run(sensor_list.passive(37e9, 55), sp)
    assert np.array_equal(a.data.values, b.data.values)


def test_error_handling(on_host):
    warm = make_snowpack([0.5, 1.0], "exponential", density=[300.0, 320.0], temperature=[260.0, 280.0], corr_length=[2e-4, 2e-4])
    fine = make_snowpack([0.5, 1.0], "exponential", density=[300.0, 320.0], temperature=[260.0, 262.0], corr_length=[2e-4, 2e-4])
    sensor = sensor_list.passive(37e9, 55)
    with pytest.raises(SMRTError, match="Invalid layer properties"):
        make_model("iba", "successive_order", rtsolver_options={"n_max_stream": 4, "n_iteration_max": 2}).run(sensor, warm)
    m = make_model("iba", "successive_order", rtsolver_options={"n_max_stream": 4, "n_iteration_max": 2, "error_handling": "nan"})
    res = m.run(sensor, [warm, fine])
    assert np.all(np.isnan(res.data.values[0])) and np.all(np.isfinite(res.data.values[1]))
    assert "optically too deep for the successive_order workspace" in _native.STATUS_MESSAGES[7]


# ---- header, binding, library ---------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_ctypes_stub
    finally:
        sys.path.pop(0)
    _, functions = gen_ctypes_stub.parse(open(os.path.join(ROOT, "include", "smrt_dort.h")).read())
    declared = {name: (ret, args) for name, ret, args in functions if name.startswith("smrt_successive_order_")}
    assert sorted(declared) == sorted(s for s in _native.EXPORTED_SYMBOLS if s.startswith("smrt_successive_order_")) and len(declared) == 8
    lib = _native.load_library()
    scope = {"C": C, "SmrtBatch": _native.SmrtBatch}
    for name, (ret, args) in declared.items():
        fn = getattr(lib, name)
        assert fn.restype is eval(ret, scope), name
        assert list(fn.argtypes) == [eval(a, scope) for a in args], name
    assert "#define SMRT_ERR_DEPTH 7" in open(os.path.join(ROOT, "include", "smrt_dort.h")).read() and 7 in _native.STATUS_MESSAGES


def test_launch_info_binding_reads_the_entry_count():
    """smrt_successive_order_launch_info returns the number of entries it has (include/smrt_dort.h), not 0: the binding
    takes a positive count as success and a negative one as the error it is."""
    class Lib:
        def __init__(self, rc):
            self.rc = rc

        def smrt_successive_order_launch_info(self, handle, info, capacity):
            for k, v in enumerate((3, 4096, 1, 8192)[:capacity]):
                info[k] = v
            return self.rc

        def smrt_dort_last_error(self, handle):
            return b"no successive-order launch to describe"

    ctx = object.__new__(_native.DortContext)
    ctx._h, ctx.lock = None, threading.RLock()
    ctx._lib = Lib(4)
    assert ctx.successive_order_launch_info() == dict(chunks=3, reserved_bytes=4096, over_budget=1, budget=8192)
    ctx._lib = Lib(-1)
    with pytest.raises(SMRTError, match="no successive-order launch to describe"):
        ctx.successive_order_launch_info()
