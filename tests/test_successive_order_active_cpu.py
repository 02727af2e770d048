"""The successive-order backscatter solver without a GPU: the NumPy restatement against every fixture, the DEVICE arithmetic
(smrt_amd/csrc/successive_order_active_kernel.hpp) compiled with g++ against every fixture, the tolerance identity and the
incident-stream selection on their own, and the Python layer (plugin, options, result labels, selectors, refusals, error
handling, binding return codes) driven end to end with the CPU build of the kernels in place of the GPU context.

Bar: every element (each order and the total, all nine polarisation pairs) within 1e-8 x the largest co-polarised total of
the fixture -- the project's active-mode contract (profiles/first_order_parity.txt) --, exact zeros exactly where the
reference has them; layer scalars: eps 1e-12, ks 1e-11, ka 1e-10 relative (tests/test_gpu_parity.py)."""
import ctypes as C
import os
import sys
import threading
import types

import numpy as np
import pytest

from host_build import host_library
from smrt_amd import _native, make_model, sensor_list
from smrt_amd.core.error import SMRTError
from smrt_amd.inputs.make_medium import make_interface, make_snowpack, make_soil
from successive_order_active_restatement import (CASES, build_snowpack, case_by_name, incident_streams, parity_bar,
                                                 pass_tolerance, solve_case, solver_options)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def api():
    return types.SimpleNamespace(make_snowpack=make_snowpack, make_soil=make_soil)


def golden(case):
    return np.load(os.path.join(GOLDEN, "successive_order_active_" + case["name"] + ".npz"))


_RESTATED = {}


def restated(case):
    """The restatement of a case, computed once and shared (never modified)."""
    if case["name"] not in _RESTATED:
        _RESTATED[case["name"]] = solve_case(case)
    return _RESTATED[case["name"]]


def assert_matches(values, reference, what):
    """values, reference [3, 3, n_theta_inc, orders + 1]; exact zeros exactly where the reference has them."""
    bar = parity_bar(reference)
    err = float(np.abs(values - reference).max())
    print(f"{what}: largest difference {err:.3e} = {err / bar * 1e-8:.2e} x the largest co-polarised total (bar 1e-8)")
    assert np.array_equal(values == 0.0, reference == 0.0), what
    assert err <= bar, (what, err, bar)
    return err / bar * 1e-8


def assert_pass_max(mine, theirs, rtol, what):
    """[passes, orders], NaN where a pass did not run the order."""
    assert np.array_equal(np.isnan(mine), np.isnan(theirs)), (what, mine, theirs)
    ran = ~np.isnan(theirs)
    assert np.all(np.abs(mine[ran] - theirs[ran]) <= rtol * np.abs(theirs[ran])), what


# ---- restatement against the fixtures -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_restatement_reproduces_the_fixture(case):
    g = golden(case)
    sol, _ = restated(case)
    assert_matches(sol["sigma"], g["sigma"], "restatement " + case["name"])
    assert np.array_equal(sol["sublayers"], g["sublayers"]) and np.array_equal(sol["streams"], g["streams"])
    mine = np.full_like(g["pass_max"], np.nan)
    for k, p in enumerate(sol["pass_max"]):
        mine[k, :len(p)] = p
    assert_pass_max(mine, g["pass_max"], 1e-12, case["name"])
    # the tolerance every pass can form from its own order 0 is the reference's, bit for bit
    rtol = case.get("relative_tolerance", 0.001)
    assert sol["tolerance"] == rtol * g["pass_max"][1, 0] or abs(sol["tolerance"] / (rtol * g["pass_max"][1, 0]) - 1) < 1e-12
    for m in range(case.get("m_max", 2) + 1):
        assert pass_tolerance(m, rtol, sol["pass_max"][1 + m][0]) == sol["tolerance"]


def test_fixtures_cover_what_they_must():
    gs = {c["name"]: golden(c) for c in CASES}
    ran = {n: (~np.isnan(g["pass_max"][1:])).sum(axis=1) for n, g in gs.items()}
    cap = {c["name"]: c["n_iteration_max"] for c in CASES}
    assert any(r.min() < cap[n] for n, r in ran.items()) and any(r.min() == cap[n] for n, r in ran.items())
    assert np.all(~np.isnan(np.concatenate([g["pass_max"][0] for g in gs.values()])))   # the coherent pass never stops
    assert any(len(set(g["streams"])) > 1 for g in gs.values())
    assert any(g["sublayers"].min() == 1 for g in gs.values()) and any(g["sublayers"].max() > 16 for g in gs.values())
    g, r = gs["iba_refraction_L3_n6"], ran["iba_refraction_L3_n6"]
    assert r.max() < 10 and np.any(g["sigma"][:, :, :, r.max():10] != 0.0)     # minus the coherent remainder after the stop
    assert np.abs(g["sigma"][:, :, :, r.max():10]).max() < 1e-3 * g["pass_max"][1, 0]   # ... bounded by the tolerance
    assert list(gs["iba_deep_L2_n8"]["sublayers"]) == [1, 294] and list(gs["iba_deep_L2_n8"]["streams"]) == [7, 8]
    assert gs["dmrt_L10_n32"]["streams"].min() == 22 and gs["dmrt_L10_n32"]["streams"].max() == 32
    assert np.all(gs["iba_soil_L2_n8"]["sigma"][:, 2] == 0.0) and np.any(gs["iba_soil_L2_n8_VHU"]["sigma"][:, 2] != 0.0)
    assert np.all(gs["iba_soil_L2_n8_V"]["sigma"][:, 1:] == 0.0)


def test_tolerance_identity():
    """At order 0 a pass sees the specular reflection of its own incident columns; mode m >= 1 carries twice mode 0's
    incident radiance, so the tolerance it forms by itself equals mode 0's bit for bit."""
    rng = np.random.default_rng(7)
    for _ in range(100):
        n_air, rtol = int(rng.integers(2, 65)), float(10.0 ** rng.uniform(-6, -1))
        R = rng.uniform(0.0, 1.0, 3 * n_air) * rng.choice([1.0, -1.0], 3 * n_air, p=[0.9, 0.1])
        power = 1.0 / (2 * np.pi * rng.uniform(1e-3, 0.3, 3 * n_air))
        mode0 = float(np.max(R * power))
        higher = float(np.max(R * (2.0 * power)))
        assert pass_tolerance(2, rtol, higher) == pass_tolerance(0, rtol, mode0) == rtol * mode0


# ---- the device source on the CPU ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_lib():
    lib = host_library("libsmrt_so_active_host.so", "successive_order_active_host.cpp")
    lib.smrt_so_active_host_run.restype = C.c_int32
    lib.smrt_so_active_host_incident.restype = C.c_int32
    return lib


def host_run(lib, batch, theta_inc, n_iteration_max, relative_tolerance, incident_npol=2, m_max=2, order=0):
    theta_inc = np.ascontiguousarray(np.atleast_1d(theta_inc), float)
    o = _native.SuccessiveOrderActiveOutput(batch, batch.n_pairs, n_iteration_max, len(theta_inc), m_max)
    rc = lib.smrt_so_active_host_run(C.byref(batch.struct), C.c_int32(n_iteration_max), C.c_double(relative_tolerance),
                                     C.c_int32(len(theta_inc)), theta_inc.ctypes.data_as(C.POINTER(C.c_double)),
                                     C.c_int32(incident_npol), C.c_int32(m_max), C.c_int32(order), *o.pointers())
    assert rc == 0
    return o


def pack_case(case):
    """The PackedBatch of a case through the solver's own packer (DORT's packing)."""
    from smrt_amd.rtsolver.successive_order_backscatter import SuccessiveOrderBackscatter

    solver = SuccessiveOrderBackscatter(**solver_options(case))
    sp = build_snowpack(case, api())
    sensor = sensor_list.active(case["frequency"], case["theta"])
    return solver._packer()._pack(sensor, [sp], np.array([case["frequency"]]), case["emmodel"]), solver, sensor


def run_case_on_host(lib, case, order=0):
    batch, solver, sensor = pack_case(case)
    return host_run(lib, batch, sensor.theta_inc, solver.n_iteration_max, solver.relative_tolerance,
                    len(solver.incident_polarizations), solver.m_max, order)


def assert_layers(out, g, L):
    lay = out.layers[0][:L]
    eps = lay[:, 0] + 1j * lay[:, 1]
    assert np.abs(eps - g["eps"]).max() <= 1e-12 * np.abs(g["eps"]).max()
    assert np.all(np.abs(lay[:, 2] - g["ks"]) <= 1e-11 * np.abs(g["ks"]))
    assert np.all(np.abs(lay[:, 3] - g["ka"]) <= 1e-10 * np.abs(g["ka"]))
    assert np.array_equal(lay[:, 4].astype(int), g["streams"]) and np.array_equal(out.sublayers[0][:L], g["sublayers"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_device_source_on_the_cpu_reproduces_the_fixture(host_lib, case):
    g = golden(case)
    out = run_case_on_host(host_lib, case)
    assert out.status[0] == 0
    assert_matches(out.values[0], g["sigma"], "device source on the CPU " + case["name"])
    assert_layers(out, g, len(case["thickness"]))
    assert_pass_max(out.max_radiance[0], g["pass_max"], 1e-10, case["name"])
    assert np.array_equal(out.orders[0], (~np.isnan(g["pass_max"])).sum(axis=1))


def test_device_source_has_no_race_between_its_phases(host_lib):
    """Fibers visited forwards, backwards and strided give the same bits: no barrier is missing in the sweep kernel."""
    case = case_by_name("iba_refraction_L3_n6")
    outs = [run_case_on_host(host_lib, case, order) for order in (0, 1, 2)]
    assert np.array_equal(outs[0].values, outs[1].values) and np.array_equal(outs[0].values, outs[2].values)


def test_incident_stream_selection(host_lib):
    """Below the smallest stream cosine: one stream; above the largest: the steepest stream alone (the nadir node is the
    interpolation's); between two streams: both."""
    outmu = np.array([0.95, 0.8, 0.55, 0.3])

    def device(theta_deg):
        theta = np.deg2rad(np.atleast_1d(np.asarray(theta_deg, float)))
        lst = np.zeros(len(outmu), np.int32)
        n = host_lib.smrt_so_active_host_incident(outmu.ctypes.data_as(C.POINTER(C.c_double)), C.c_int32(len(outmu)),
                                                  theta.ctypes.data_as(C.POINTER(C.c_double)), C.c_int32(len(theta)),
                                                  lst.ctypes.data_as(C.POINTER(C.c_int32)))
        return list(lst[:n])

    steep, between, grazing = 10.0, 45.0, 80.0     # cosines 0.985, 0.707, 0.174
    assert device(grazing) == incident_streams(outmu, grazing) == [3]
    assert device(steep) == incident_streams(outmu, steep) == [0]
    assert device(between) == incident_streams(outmu, between) == [1, 2]
    assert device([steep, between, grazing]) == incident_streams(outmu, [steep, between, grazing]) == [0, 1, 2, 3]
    assert device([between, 40.0]) == incident_streams(outmu, [between, 40.0]) == [1, 2]


def test_nadir_insertion_and_single_stream(host_lib):
    """An incidence angle steeper than the steepest stream interpolates from the nadir node; one grazing angle alone selects one
    stream and the answer is that stream's.  Against the restatement (the reference's arithmetic)."""
    case = dict(case_by_name("iba_soil_L2_n8"), n_iteration_max=3)
    for theta in ([5.0, 30.0], [85.0], [5.0]):
        c = dict(case, theta=theta)
        sol, _ = solve_case(c)
        out = run_case_on_host(host_lib, c)
        assert out.status[0] == 0
        assert_matches(out.values[0], sol["sigma"], f"device source on the CPU, theta_inc {theta}")


# ---- the Python layer, end to end on the CPU build of the kernels ---------------------------------------------------------
class HostContext:
    """Stands in for DortContext: the same calls, answered by the CPU build of the device source."""

    def __init__(self, lib):
        self.lib, self.lock, self.calls = lib, threading.RLock(), 0

    def so_active_run(self, batch, theta_inc, n_iteration_max=50, relative_tolerance=0.001, incident_npol=2, m_max=2, pairs=None,
                      workspace_budget=None):
        self.calls += 1
        o = host_run(self.lib, batch, theta_inc, n_iteration_max, relative_tolerance, incident_npol, m_max)
        if pairs is not None:
            for name in ("values", "status", "layers", "streams", "sublayers", "max_radiance", "orders"):
                setattr(o, name, getattr(o, name)[np.asarray(pairs)])
        return o

    def so_active_launch_info(self):
        return dict(chunks=1, reserved_bytes=0, over_budget=0, budget=0)


@pytest.fixture()
def on_host(host_lib, monkeypatch):
    from smrt_amd.rtsolver import successive_order_backscatter as module

    ctx = HostContext(host_lib)
    monkeypatch.setattr(module, "get_context", lambda device=None: ctx)
    return ctx


def test_plugin_resolution_and_options():
    from smrt_amd.core.plugin import import_class
    from smrt_amd.rtsolver.successive_order_backscatter import SuccessiveOrderBackscatter

    assert import_class("rtsolver", "successive_order_backscatter") is SuccessiveOrderBackscatter
    m = make_model("iba", "successive_order_backscatter", rtsolver_options={"n_max_stream": 8, "n_iteration_max": 12, "m_max": 1})
    solver = m.make_rtsolver_instance()
    assert isinstance(solver, SuccessiveOrderBackscatter) and (solver.n_max_stream, solver.n_iteration_max, solver.m_max) == (8, 12, 1)
    d = SuccessiveOrderBackscatter()
    assert (d.n_max_stream, d.n_iteration_max, d.relative_tolerance, d.m_max, d.stream_mode, d.incident_polarizations) == \
        (32, 50, 0.001, 2, "most_refringent", "VH")
    for bad in (dict(phase_symmetrization=True), dict(process_coherent_layers=True), dict(error_handling="ignore"),
                dict(stream_mode="uniform_air"), dict(n_max_stream=1), dict(n_max_stream=65), dict(n_iteration_max=0),
                dict(relative_tolerance=-1.0), dict(incident_polarizations="H")):
        with pytest.raises(SMRTError):
            SuccessiveOrderBackscatter(**bad)


def test_done_when_example(on_host):
    case = case_by_name("iba_soil_L2_n8")
    sp = build_snowpack(case, api())
    m = make_model("iba", "successive_order_backscatter", rtsolver_options=solver_options(case))
    res = m.run(sensor_list.active(13e9, [30, 50]), sp)
    g = golden(case)["sigma"]
    assert res.data.dims == ("polarization_inc", "polarization", "theta_inc", "order") and res.data.shape == (3, 3, 2, 9)
    assert list(res.data.coords["order"]) == list(range(8)) + ["total"]
    assert_matches(np.asarray(res.data.values), g, "Model.run on the CPU build")
    scale = 4 * np.pi * np.cos(np.deg2rad([30.0, 50.0]))
    bar = parity_bar(g) * scale.max()
    assert np.abs(np.asarray(res.sigmaVV(order="total")) - scale * g[0, 0, :, -1]).max() <= bar
    assert np.abs(np.asarray(res.sigmaHH(order=1)) - scale * g[1, 1, :, 1]).max() <= bar
    assert np.abs(np.asarray(res.sigmaVV(order=0))).max() == 0.0       # the coherent part is removed
    hv = np.asarray(res.sigmaHV_dB(order=2))
    assert hv.shape == (2,) and np.all(np.isfinite(hv))
    assert np.allclose(hv, 10 * np.log10(np.asarray(res.sigmaHV(order=2))))
    other = res.other_data
    assert set(other) >= {"stream_angles", "effective_permittivity", "ks", "ka", "ke", "thickness"}
    assert np.allclose(other["thickness"].values, case["thickness"]) and other["ks"].values.shape == (2,)


def test_model_run_batches_into_one_launch_per_group(on_host):
    soil = make_soil("flat", complex(5.0, 0.5), 265.0)
    sps = [make_snowpack([0.2, 0.4 + 0.1 * k], "exponential", density=[250.0, 350.0], temperature=[255.0, 262.0],
                         corr_length=[2e-4, 4e-4], substrate=soil if k % 2 else None) for k in range(4)]
    m = make_model("iba", "successive_order_backscatter", rtsolver_options={"n_max_stream": 4, "n_iteration_max": 3})
    res = m.run(sensor_list.active([13e9, 17e9], 35), sps)
    assert on_host.calls == 2          # with and without substrate
    assert res.data.dims == ("frequency", "snowpack", "polarization_inc", "polarization", "theta_inc", "order")
    assert res.data.shape == (2, 4, 3, 3, 1, 4)
    single = m.run(sensor_list.active(17e9, 35), sps[1])
    assert np.array_equal(single.data.values, res.data.values[1, 1])
    solver = m.make_rtsolver_instance()
    out = solver.solve_batch([(sensor_list.active(13e9, 35), sps[0]), (sensor_list.active(13e9, [35, 45]), sps[0])], "iba")
    assert solver.launches == 2 and len(solver.launch_info) == 2 and out[1].data.shape == (3, 3, 2, 4)


def test_out_of_scope_inputs_raise(on_host):
    from smrt_amd.atmosphere.simple_isotropic_atmosphere import SimpleIsotropicAtmosphere
    from smrt_amd.rtsolver.successive_order_backscatter import SuccessiveOrderBackscatter
    from smrt_amd.substrate.reflector import make_reflector
    from smrt_amd.substrate.transparent import Transparent

    kw = dict(density=[300.0], temperature=[260.0], corr_length=[2e-4])
    sp = make_snowpack([1.0], "exponential", **kw)
    radar = sensor_list.active(13e9, 30)
    m = make_model("iba", "successive_order_backscatter", rtsolver_options={"n_max_stream": 4, "n_iteration_max": 2})
    with pytest.raises(SMRTError, match="use rtsolver 'successive_order' for passive sensors"):
        m.run(sensor_list.passive(37e9, 55), sp)
    with pytest.raises(SMRTError, match="active sensors.*use rtsolver 'successive_order_backscatter'"):
        make_model("iba", "successive_order").run(radar, sp)
    atmosphere = SimpleIsotropicAtmosphere(tb_down=20.0, tb_up=18.0, transmittance=0.9)
    with pytest.raises(SMRTError, match="can not handle atmosphere yet."):
        m.run(radar, atmosphere + sp)
    with pytest.raises(SMRTError, match="can not handle atmosphere yet."):
        SuccessiveOrderBackscatter().solve(sp, [None], radar, atmosphere=atmosphere)
    rough = make_snowpack([1.0], "exponential", interface=[make_interface("geometrical_optics_backscatter", mean_square_slope=0.03)], **kw)
    with pytest.raises(SMRTError, match="rough interfaces"):
        m.run(radar, rough)
    rough_soil = make_snowpack([1.0], "exponential", substrate=make_soil("geometrical_optics_backscatter", complex(8.0, 1.0), 268.0,
                                                                        mean_square_slope=0.05), **kw)
    with pytest.raises(SMRTError, match="substrate"):
        m.run(radar, rough_soil)
    mirror = make_snowpack([1.0], "exponential", substrate=make_reflector(temperature=265.0, specular_reflection=dict(V=0.6, H=0.7)), **kw)
    with pytest.raises(SMRTError, match="Reflector is not implemented"):
        m.run(radar, mirror)
    with pytest.raises(SMRTError, match="evaluated on the host"):
        make_model("rayleigh", "successive_order_backscatter", rtsolver_options={"n_max_stream": 4}).run(
            radar, make_snowpack([1.0], "sticky_hard_spheres", density=[300.0], temperature=[260.0], radius=[2e-4], stickiness=[0.2]))
    for option in ("process_coherent_layers", "phase_symmetrization"):
        with pytest.raises(SMRTError, match=option):
            make_model("iba", "successive_order_backscatter", rtsolver_options={option: True}).run(radar, sp)
    with pytest.raises(SMRTError, match="most_refringent"):
        make_model("iba", "successive_order_backscatter", rtsolver_options={"stream_mode": "uniform_air"}).run(radar, sp)
    with pytest.raises(SMRTError, match="phi as an array must be implemented"):
        m.run(sensor_list.active(13e9, 30, phi=[0.0, 180.0]), sp)
    # a transparent substrate is no substrate
    clear = make_snowpack([1.0], "exponential", substrate=Transparent(), **kw)
    assert np.array_equal(m.run(radar, clear).data.values, m.run(radar, sp).data.values)


def test_error_handling(on_host):
    warm = make_snowpack([0.5, 1.0], "exponential", density=[300.0, 320.0], temperature=[260.0, 280.0], corr_length=[2e-4, 2e-4])
    fine = make_snowpack([0.5, 1.0], "exponential", density=[300.0, 320.0], temperature=[260.0, 262.0], corr_length=[2e-4, 2e-4])
    radar = sensor_list.active(13e9, 35)
    options = {"n_max_stream": 4, "n_iteration_max": 2}
    with pytest.raises(SMRTError, match="Invalid layer properties"):
        make_model("iba", "successive_order_backscatter", rtsolver_options=options).run(radar, warm)
    m = make_model("iba", "successive_order_backscatter", rtsolver_options=dict(options, error_handling="nan"))
    res = m.run(radar, [warm, fine])
    assert np.all(np.isnan(res.data.values[0])) and np.all(np.isfinite(res.data.values[1]))


# ---- header, binding, library ---------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_ctypes_stub
    finally:
        sys.path.pop(0)
    _, functions = gen_ctypes_stub.parse(open(os.path.join(ROOT, "include", "smrt_dort.h")).read())
    declared = {name: (ret, args) for name, ret, args in functions if name.startswith("smrt_so_active_")}
    assert sorted(declared) == sorted(s for s in _native.EXPORTED_SYMBOLS if s.startswith("smrt_so_active_")) and len(declared) == 8
    lib = _native.load_library()
    scope = {"C": C, "SmrtBatch": _native.SmrtBatch}
    for name, (ret, args) in declared.items():
        fn = getattr(lib, name)
        assert fn.restype is eval(ret, scope), name
        assert list(fn.argtypes) == [eval(a, scope) for a in args], name


class _Lib:
    """Stand-in library: records the calls, answers with the configured return codes."""

    def __init__(self, info_rc=4, rc=0):
        self.info_rc, self.rc, self.calls = info_rc, rc, []

    def smrt_so_active_launch_info(self, handle, info, capacity):
        for k, v in enumerate((3, 4096, 1, 8192)[:capacity]):
            info[k] = v
        return self.info_rc

    def smrt_dort_last_error(self, handle):
        return b"no successive-order backscatter launch to describe"

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            return self.rc
        return call


def _context(lib):
    ctx = object.__new__(_native.DortContext)
    ctx._h, ctx.lock = None, threading.RLock()
    ctx._lib = lib
    return ctx


def test_launch_info_binding_reads_the_entry_count():
    """smrt_so_active_launch_info returns the number of entries it has (include/smrt_dort.h), not 0: the binding takes a
    positive count as success and a negative one as the error it is."""
    assert _context(_Lib(4)).so_active_launch_info() == dict(chunks=3, reserved_bytes=4096, over_budget=1, budget=8192)
    with pytest.raises(SMRTError, match="no successive-order backscatter launch to describe"):
        _context(_Lib(-1)).so_active_launch_info()


def test_binding_return_codes():
    batch, solver, sensor = pack_case(case_by_name("iba_L1_n4"))
    ok = _context(_Lib(rc=0))
    out = ok.so_active_run(batch, sensor.theta_inc, 6, 0.001, incident_npol=2, m_max=2)
    assert out.values.shape == (1, 3, 3, 1, 7) and out.max_radiance.shape == (1, 4, 6) and out.orders.shape == (1, 4)
    ok.so_active_upload(batch, sensor.theta_inc, 6, 0.001)
    ok.so_active_launch(), ok.so_active_sync()
    assert ok.so_active_download().values.shape == (1, 3, 3, 1, 7) and len(ok.so_active_kernel_ms()) == 3
    assert ok._lib.calls == ["smrt_so_active_run_pairs", "smrt_so_active_upload_pairs", "smrt_so_active_launch", "smrt_so_active_sync",
                             "smrt_so_active_download", "smrt_so_active_kernel_ms"]
    failing = _context(_Lib(rc=-1))
    for call in (lambda: failing.so_active_run(batch, sensor.theta_inc, 6, 0.001), lambda: failing.so_active_upload(batch, sensor.theta_inc),
                 failing.so_active_launch, failing.so_active_sync, failing.so_active_kernel_ms):
        with pytest.raises(SMRTError):
            call()
