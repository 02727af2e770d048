"""The multi-Fresnel thermal emission solver without a GPU: the NumPy restatement against every fixture, the DEVICE arithmetic
(smrt_amd/csrc/multifresnel_kernel.hpp) compiled with g++ against every fixture and against the restatement, and the Python
layer (plugin, options, result labels, refusals, warnings, error handling) driven end to end with the CPU build of the kernels
in place of the GPU context.

Tolerances: 1e-6 K for every brightness temperature (TB_ATOL, the project's bar); layer scalars: eps 1e-12, ks 1e-11, ka 1e-10
relative (tests/test_gpu_parity.py); layers_used exactly; tau_snowpack 1e-12 relative.  Measured: profiles/multifresnel_parity.txt."""
import ctypes as C
import os
import threading
import types
import warnings

import numpy as np
import pytest

from host_build import host_library
from smrt_amd import _native, make_model, sensor_list
from smrt_amd.core.error import SMRTError, SMRTWarning
from smrt_amd.inputs.make_medium import make_interface, make_snowpack, make_soil
from multifresnel_restatement import CASES, TB_ATOL, build_snowpack, case_by_name, solve_case, solver_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
IDS = dict(ids=lambda c: c["name"])


def api():
    return types.SimpleNamespace(make_snowpack=make_snowpack, make_soil=make_soil)


def golden(case):
    return np.load(os.path.join(GOLDEN, "multifresnel_" + case["name"] + ".npz"))


_RESTATED = {}


def restated(case):
    """The restatement of a case, computed once and shared (never modified)."""
    if case["name"] not in _RESTATED:
        _RESTATED[case["name"]] = solve_case(case)
    return _RESTATED[case["name"]]


def assert_tb(values, reference, what):
    err = float(np.abs(values - reference).max())
    print(f"{what}: largest difference {err:.3e} K (bar {TB_ATOL:g})")
    assert np.all(np.isfinite(values)) and err <= TB_ATOL, (what, err)


# ---- restatement against the fixtures -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, **IDS)
def test_restatement_reproduces_the_fixture(case):
    g = golden(case)
    sol, layers = restated(case)
    assert_tb(sol["tb"], g["tb"], "restatement " + case["name"])
    assert sol["layers_used"] == int(g["layers_used"])
    assert abs(sol["tau_snowpack"] - float(g["tau_snowpack"])) <= 1e-12 * float(g["tau_snowpack"])
    assert np.array_equal(sol["first_clipped"], g["first_clipped"])
    eps = np.array([lay.eps_eff for lay in layers])
    assert np.abs(eps - g["eps"]).max() <= 1e-12 * np.abs(g["eps"]).max()


def test_fixtures_cover_what_they_can():
    """What the fixtures exercise -- and what no fixture of this reference can: its stop needs a negative remainder and the
    remainder is x - clip(tau, 0, x) >= 0, so every case uses all its layers (tests/multifresnel_restatement.py)."""
    gs = {c["name"]: golden(c) for c in CASES}
    slots = {c["name"]: len(gs[c["name"]]["ks"]) + (1 if "substrate" in c else 0) for c in CASES}
    assert all(int(g["layers_used"]) == slots[n] for n, g in gs.items())
    assert all(np.all(np.isfinite(g["tb"])) for g in gs.values())
    p1 = gs["firn_prune1"]
    assert abs(float(p1["tau_snowpack"]) - 1.0) < 1e-14                       # the steepest angle runs out ...
    assert np.all(p1["first_clipped"] > 0) and np.all(p1["first_clipped"] < 299)
    assert np.all(np.diff(p1["first_clipped"]) < 0)                           # ... after the oblique ones, in order
    assert all(np.all(gs[n]["first_clipped"] == -1) for n in ("L1", "firn_L300_19GHz", "firn_noprune", "iba_L4", "firn_L4000"))
    assert np.array_equal(gs["firn_noprune"]["tb"], gs["firn_L300_19GHz"]["tb"])   # tau = 1.41 < 10: the default never clips it
    assert np.abs(gs["firn_prune1"]["tb"] - gs["firn_L300_19GHz"]["tb"]).min() > 20.0
    assert all(r["remainders"].min() >= 0.0 for r in (restated(c)[0] for c in CASES if c["name"] != "firn_noprune"))
    for name in ("soil_L3", "firn_prune1", "soil_lossless"):
        assert restated(case_by_name(name))[0]["remainders"][-1] == 0.0      # exhausted exactly, never below


# ---- the device source on the CPU ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_lib():
    lib = host_library("libsmrt_multifresnel_host.so", "multifresnel_host.cpp")
    lib.smrt_multifresnel_host_run.restype = C.c_int32
    return lib


def host_run(lib, batch, mu, prune_deep_snowpack):
    mu = np.ascontiguousarray(mu, float)
    o = _native.MultiFresnelOutput(batch, batch.n_pairs, mu)
    none = prune_deep_snowpack is None
    rc = lib.smrt_multifresnel_host_run(C.byref(batch.struct), mu.ctypes.data_as(C.POINTER(C.c_double)),
                                        C.c_double(0.0 if none else prune_deep_snowpack), C.c_int32(1 if none else 0), *o.pointers())
    assert rc == 0
    return o


def pack_case(case):
    """The PackedBatch of a case through the solver's own packer (DORT's packing)."""
    from smrt_amd.rtsolver.multifresnel_thermalemission import MultiFresnelThermalEmission

    solver = MultiFresnelThermalEmission(**solver_options(case))
    sp = build_snowpack(case, api())
    sensor = sensor_list.passive(case["frequency"], case["theta"])
    return solver._packer()._pack(sensor, [sp], np.array([case["frequency"]]), case["emmodel"]), solver, sensor


def assert_output(out, g, what):
    assert np.all(out.status[0] == 0)
    assert_tb(out.values[0], g["tb"], what)
    L = len(g["ks"])
    lay = out.layers[0][:L]
    assert np.abs(lay[:, 0] + 1j * lay[:, 1] - g["eps"]).max() <= 1e-12 * np.abs(g["eps"]).max()
    assert np.all(np.abs(lay[:, 2] - g["ks"]) <= 1e-11 * np.abs(g["ks"])) and np.all(np.abs(lay[:, 3] - g["ka"]) <= 1e-10 * np.abs(g["ka"]))
    assert out.layers_used[0] == int(g["layers_used"])
    assert abs(out.tau_snowpack[0] - float(g["tau_snowpack"])) <= 1e-12 * float(g["tau_snowpack"])


@pytest.mark.parametrize("case", CASES, **IDS)
def test_device_source_on_the_cpu_reproduces_the_fixture_and_the_restatement(host_lib, case):
    batch, solver, sensor = pack_case(case)
    out = host_run(host_lib, batch, np.cos(sensor.theta), solver.prune_deep_snowpack)
    assert_output(out, golden(case), "device source on the CPU " + case["name"])
    assert_tb(out.values[0], restated(case)[0]["tb"], "device source against the restatement " + case["name"])


def test_iba_layers_give_the_tb_of_nonscattering_layers(host_lib):
    case = case_by_name("iba_L4")
    batch, solver, sensor = pack_case(case)
    plain, _, _ = pack_case(dict(case, emmodel="nonscattering"))
    a = host_run(host_lib, batch, np.cos(sensor.theta), 10)
    b = host_run(host_lib, plain, np.cos(sensor.theta), 10)
    assert np.abs(a.values - b.values).max() <= TB_ATOL and np.all(a.layers[0][:, 2] > 0.0) and np.all(b.layers[0][:, 2] == 0.0)


def test_grazing_angle_is_non_finite_in_the_restatement_and_gets_a_status_word(host_lib):
    """theta = 90 degrees: the reflectivity of the surface is exactly 1 and 1 / (1 - r) divides by zero."""
    from multifresnel_restatement import multifresnel, oracle_layers, profile

    case = dict(case_by_name("soil_L3"), theta=[10.0, 90.0, 50.0])
    p = profile(case)
    sol = multifresnel([lay.eps_eff for lay in oracle_layers(case)], p["temperature"], p["thickness"], case["frequency"], case["theta"])
    assert not np.any(np.isfinite(sol["tb"][1])) and np.all(np.isfinite(sol["tb"][[0, 2]]))
    batch, solver, sensor = pack_case(case)
    out = host_run(host_lib, batch, np.cos(sensor.theta), 10)
    assert list(out.status[0]) == [0, 8, 0] and np.all(np.isnan(out.values[0][1])) and np.all(np.isfinite(out.values[0][[0, 2]]))
    assert_tb(out.values[0][[0, 2]], golden(case_by_name("soil_L3"))["tb"], "neighbours of the grazing angle")


def test_grazing_angle_is_non_finite_whatever_the_permittivity(host_lib):
    """The reflectivity at 90 degrees is (k - 0) / (0 + k) squared, and the device divides so that this is exactly 1 for every
    k (mf_cdiv).  A division through a rounded reciprocal leaves 1 -+ 1 ulp for about one permittivity in seven and a finite
    Tb of the order of 1e16 K; so does NumPy's in the restatement and the reference, which is why only the device source is
    held to this."""
    rng = np.random.RandomState(7)
    sps = [make_snowpack([d], "exponential", density=[rho], temperature=[T], corr_length=1e-4)
           for d, rho, T in zip(rng.uniform(0.05, 2.0, 150), rng.uniform(200.0, 900.0, 150), rng.uniform(235.0, 270.0, 150))]
    from smrt_amd.rtsolver.multifresnel_thermalemission import MultiFresnelThermalEmission

    frequencies = np.array([1.4e9, 19e9])
    theta = [5.0, 90.0, 60.0]
    batch = MultiFresnelThermalEmission()._packer()._pack(sensor_list.passive(frequencies, theta), sps, frequencies, "nonscattering")
    out = host_run(host_lib, batch, np.cos(np.deg2rad(theta)), 10)
    assert out.status.shape == (300, 3) and np.array_equal(out.status, np.broadcast_to([0, 8, 0], (300, 3)))
    assert np.all(np.isnan(out.values[:, 1])) and np.all(np.isfinite(out.values[:, [0, 2]]))


# ---- the Python layer, end to end on the CPU build of the kernels ---------------------------------------------------------
class HostContext:
    """Stands in for DortContext: the same call, answered by the CPU build of the device source."""

    def __init__(self, lib):
        self.lib, self.lock, self.calls = lib, threading.RLock(), 0

    def multifresnel_run(self, batch, mu, prune_deep_snowpack=10, pairs=None):
        self.calls += 1
        o = host_run(self.lib, batch, mu, prune_deep_snowpack)
        if pairs is not None:
            for name in ("values", "status", "layers_used", "tau_snowpack", "layers", "streams"):
                setattr(o, name, getattr(o, name)[np.asarray(pairs)])
        return o


@pytest.fixture()
def on_host(host_lib, monkeypatch):
    from smrt_amd.rtsolver import multifresnel_thermalemission as module

    ctx = HostContext(host_lib)
    monkeypatch.setattr(module, "get_context", lambda device=None: ctx)
    return ctx


def test_plugin_resolution_and_options():
    from smrt_amd.core.plugin import import_class
    from smrt_amd.rtsolver.multifresnel_thermalemission import MultiFresnelThermalEmission

    assert import_class("rtsolver", "multifresnel_thermalemission") is MultiFresnelThermalEmission
    m = make_model("nonscattering", "multifresnel_thermalemission", rtsolver_options={"prune_deep_snowpack": 3, "error_handling": "nan"})
    solver = m.make_rtsolver_instance()
    assert isinstance(solver, MultiFresnelThermalEmission) and solver.prune_deep_snowpack == 3.0 and solver.error_handling == "nan"
    d = MultiFresnelThermalEmission()
    assert (d.error_handling, d.prune_deep_snowpack, d.devices, d.launches) == ("exception", 10.0, None, 0)
    assert MultiFresnelThermalEmission(prune_deep_snowpack=None).prune_deep_snowpack is None
    assert MultiFresnelThermalEmission._broadcast_capability == {"theta", "polarization"}
    for bad in (dict(error_handling="ignore"), dict(prune_deep_snowpack=-1), dict(prune_deep_snowpack="deep"),
                dict(prune_deep_snowpack=float("nan")), dict(prune_deep_snowpack=True)):
        with pytest.raises(SMRTError):
            MultiFresnelThermalEmission(**bad)
    assert [a for a, _ in m.split_axes(sensor_list.passive([1.4e9, 19e9], [40, 55]))] == ["frequency"]


@pytest.mark.parametrize("case", CASES, **IDS)
def test_model_run_reproduces_the_fixture(on_host, case):
    g = golden(case)
    m = make_model(case["emmodel"], "multifresnel_thermalemission", rtsolver_options=solver_options(case))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", SMRTWarning)
        res = m.run(sensor_list.passive(case["frequency"], case["theta"]), build_snowpack(case, api()))
    assert res.data.dims == ("theta", "polarization") and list(res.data.coords["polarization"]) == ["V", "H"]
    assert np.allclose(res.data.coords["theta"], case["theta"])
    assert_tb(res.data.values, g["tb"], "Model.run " + case["name"])
    assert_tb(np.ravel(res.TbV()), g["tb"][:, 0], "TbV")
    assert_tb(np.ravel(res.TbH()), g["tb"][:, 1], "TbH")
    other = res.other_data
    assert set(other) >= {"effective_permittivity", "ks", "ka", "ke", "thickness"}
    assert np.allclose(other["ke"].values, other["ks"].values + other["ka"].values) and len(other["thickness"].values) == len(g["ks"])
    assert np.all(np.abs(other["ka"].values - g["ka"]) <= 1e-10 * np.abs(g["ka"]))


def test_model_run_batches_into_one_launch_per_group(on_host):
    soil = make_soil("flat", complex(5.0, 0.5), 270.0)
    sps = [make_snowpack([0.2, 0.4 + 0.1 * k, 50.0][:2 + k % 2], "exponential", density=[250.0, 350.0, 400.0][:2 + k % 2],
                         temperature=[255.0, 262.0, 260.0][:2 + k % 2], corr_length=1e-4, substrate=soil if k % 2 else None)
           for k in range(4)]
    m = make_model("nonscattering", "multifresnel_thermalemission")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", SMRTWarning)
        res = m.run(sensor_list.passive([1.4e9, 19e9], [30, 53]), sps)
        assert on_host.calls == 2          # with and without substrate
        assert res.data.dims == ("frequency", "snowpack", "theta", "polarization") and res.data.shape == (2, 4, 2, 2)
        single = m.run(sensor_list.passive(19e9, [30, 53]), sps[1])
    assert np.array_equal(single.data.values, res.data.values[1, 1])


def test_out_of_scope_inputs_raise(on_host):
    from smrt_amd.atmosphere.simple_isotropic_atmosphere import SimpleIsotropicAtmosphere
    from smrt_amd.rtsolver.multifresnel_thermalemission import MultiFresnelThermalEmission
    from smrt_amd.substrate.reflector import make_reflector

    kw = dict(density=[300.0], temperature=[260.0], corr_length=[2e-4])
    sp = make_snowpack([1000.0], "exponential", **kw)
    m = make_model("nonscattering", "multifresnel_thermalemission")
    sensor = sensor_list.passive(19e9, 55)
    with pytest.raises(SMRTError, match="only suitable for passive microwave"):
        m.run(sensor_list.active(13e9, 30), sp)
    atmosphere = SimpleIsotropicAtmosphere(tb_down=20.0, tb_up=18.0, transmittance=0.9)
    with pytest.raises(SMRTError, match="can not handle atmosphere"):
        m.run(sensor, atmosphere + sp)
    with pytest.raises(SMRTError, match="can not handle atmosphere"):
        MultiFresnelThermalEmission().solve(sp, [None], sensor, atmosphere=atmosphere)
    rough = make_snowpack([1000.0], "exponential", interface=[make_interface("geometrical_optics_backscatter", mean_square_slope=0.03)], **kw)
    with pytest.raises(SMRTError, match="flat interfaces"):
        m.run(sensor, rough)
    for substrate in (make_soil("geometrical_optics_backscatter", complex(8.0, 1.0), 268.0, mean_square_slope=0.05),
                      make_reflector(temperature=265.0, specular_reflection=0.5)):
        with pytest.raises(SMRTError, match="flat substrates"):
            m.run(sensor, make_snowpack([1000.0], "exponential", substrate=substrate, **kw))
    with pytest.raises(SMRTError, match="does not broadcast the frequency"):
        MultiFresnelThermalEmission().solve_batch([(sensor_list.passive([19e9, 37e9], 55), sp)], "nonscattering")
    with pytest.raises(SMRTError, match="evaluated on the host"):
        make_model("rayleigh", "multifresnel_thermalemission").run(
            sensor, make_snowpack([1000.0], "sticky_hard_spheres", density=[300.0], temperature=[260.0], radius=[2e-4], stickiness=[0.2]))


def test_warnings_once_per_run_with_counts(on_host):
    from smrt_amd.substrate.transparent import Transparent

    kw = dict(density=[300.0, 350.0], temperature=[258.0, 260.0], corr_length=1e-4)
    shallow = [make_snowpack([0.5, 1.0 + k], "exponential", **kw) for k in range(3)]
    deep = make_snowpack([0.5, 3000.0], "exponential", **kw)
    clear = make_snowpack([0.5, 1.0], "exponential", substrate=Transparent(), **kw)
    lossless = [make_snowpack([0.5, 1.0], "exponential", substrate=make_soil("flat", complex(5.0, 1e-9), 270.0), **kw) for _ in range(2)]
    lossy = make_snowpack([0.5, 1.0], "exponential", substrate=make_soil("flat", complex(5.0, 0.5), 270.0), **kw)
    m = make_model("nonscattering", "multifresnel_thermalemission")
    sensor = sensor_list.passive(19e9, [40, 55])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = m.run(sensor, shallow + [deep, clear] + lossless + [lossy])
    texts = [str(w.message) for w in caught if issubclass(w.category, SMRTWarning)]
    assert len(texts) == 2
    assert any("too small imaginary part for reliable results (2 simulation(s))" in t for t in texts)
    assert any("optically shallow in 3 simulation(s)" in t and "add a transparent substrate to supress this warning" in t for t in texts)
    # the transparent substrate is no substrate: the Tb of the same snowpack without one
    assert np.array_equal(res.data.values[4], res.data.values[0])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        m.run(sensor, [deep, clear, lossy])
    assert not [w for w in caught if issubclass(w.category, SMRTWarning)]


def test_error_handling(on_host):
    kw = dict(density=[300.0, 320.0], corr_length=1e-4)
    warm = make_snowpack([0.5, 2000.0], "exponential", temperature=[260.0, 280.0], **kw)
    fine = make_snowpack([0.5, 2000.0], "exponential", temperature=[260.0, 262.0], **kw)
    with pytest.raises(SMRTError, match="Invalid layer properties"):
        make_model("nonscattering", "multifresnel_thermalemission").run(sensor_list.passive(19e9, 55), warm)
    m = make_model("nonscattering", "multifresnel_thermalemission", rtsolver_options={"error_handling": "nan"})
    res = m.run(sensor_list.passive(19e9, [40, 55]), [warm, fine])
    assert np.all(np.isnan(res.data.values[0])) and np.all(np.isfinite(res.data.values[1]))
    # one element: the grazing angle of one simulation; its neighbours are untouched
    res = m.run(sensor_list.passive(19e9, [40, 90, 55]), [fine])
    assert np.all(np.isnan(res.data.values[0][1])) and np.all(np.isfinite(res.data.values[0][[0, 2]]))
    with pytest.raises(SMRTError, match="non-finite brightness temperature"):
        make_model("nonscattering", "multifresnel_thermalemission").run(sensor_list.passive(19e9, [40, 90, 55]), fine)


# ---- header, binding, library ---------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_ctypes_stub
    finally:
        sys.path.pop(0)
    header = open(os.path.join(ROOT, "include", "smrt_dort.h")).read()
    _, functions = gen_ctypes_stub.parse(header)
    declared = {name: (ret, args) for name, ret, args in functions if name.startswith("smrt_multifresnel_")}
    assert sorted(declared) == sorted(s for s in _native.EXPORTED_SYMBOLS if s.startswith("smrt_multifresnel_")) and len(declared) == 7
    lib = _native.load_library()
    scope = {"C": C, "SmrtBatch": _native.SmrtBatch}
    for name, (ret, args) in declared.items():
        fn = getattr(lib, name)
        assert fn.restype is eval(ret, scope), name
        assert list(fn.argtypes) == [eval(a, scope) for a in args], name
    assert "#define SMRT_ERR_NONFINITE 8" in header and 8 in _native.STATUS_MESSAGES


def test_binding_fails_on_negative_return_codes_only():
    """include/smrt_dort.h: negative means error.  A stand-in library shows the binding passes 0 and a positive value and
    raises the library's message on a negative one."""
    class Lib:
        def __init__(self, rc):
            self.rc, self.seen = rc, None

        def smrt_multifresnel_run_pairs(self, handle, batch, mu, prune, none, pairs, n_pairs, out, status, used, tau, layers):
            self.seen = (prune, none, n_pairs)
            out[0], out[1], status[0], used[0], tau[0] = 250.0, 240.0, 0, 3, 1.5
            return self.rc

        def smrt_multifresnel_kernel_ms(self, handle, ms2):
            ms2[0], ms2[1] = 0.25, 0.5
            return self.rc

        def smrt_dort_last_error(self, handle):
            return b"no multi-Fresnel batch uploaded"

    batch = _native.PackedBatch([1], [1.0], [0.3], [260.0], [1e-4], None, [1.4e9], [0.0], emmodel="nonscattering")
    ctx = object.__new__(_native.DortContext)
    ctx._h, ctx.lock = None, threading.RLock()
    for rc in (0, 2):
        ctx._lib = Lib(rc)
        out = ctx.multifresnel_run(batch, [1.0], None)
        assert ctx._lib.seen == (0.0, 1, -1) and list(out.values[0, 0]) == [250.0, 240.0] and out.layers_used[0] == 3
        assert ctx.multifresnel_kernel_ms() == (0.25, 0.5)
        ctx.multifresnel_run(batch, [1.0], 7, pairs=[0])
        assert ctx._lib.seen == (7.0, 0, 1)
    ctx._lib = Lib(-1)
    with pytest.raises(SMRTError, match="smrt_multifresnel_run_pairs failed: no multi-Fresnel batch uploaded"):
        ctx.multifresnel_run(batch, [1.0], 10)
    with pytest.raises(SMRTError, match="no multi-Fresnel batch uploaded"):
        ctx.multifresnel_kernel_ms()
    with pytest.raises(SMRTError, match="one sensor cosine per angle"):
        ctx.multifresnel_run(batch, [1.0, 0.5], 10)
