"""The nadir LRM altimetry solver without a GPU: the NumPy restatement against every fixture, the DEVICE arithmetic
(smrt_amd/csrc/nadir_lrm_altimetry_kernel.hpp) compiled with g++ against every fixture and against the restatement, the sensor
list against its fixture, and the Python layer (plugin, options, dims, coords, refusals, error handling, save / open_result)
driven end to end with the CPU build of the kernels in place of the GPU context.

Bars: every waveform sample of every contribution within 1e-8 x the peak of the case's total waveform; layer scalars eps 1e-12,
ke 1e-10, backward scattering 1e-10 relative (tests/test_gpu_parity.py's bars for eps, ka and ks); z_gate, delay, gate 1e-12
relative.  Measured: profiles/nadir_lrm_altimetry_parity.txt."""
import ctypes as C
import os
import threading
import types

import numpy as np
import pytest

from host_build import host_library
from smrt_amd import _native, make_model
from smrt_amd.core.error import SMRTError
from smrt_amd.core.result import AltimetryResult, open_result
from smrt_amd.inputs import lrm_altimeter_list
from smrt_amd.inputs.make_medium import make_interface, make_snowpack, make_soil
from nadir_lrm_altimetry_restatement import CASES, REL_BAR, SMALL, build_snowpack, case_by_name, make_sensor, solve_case, solver_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
IDS = dict(ids=lambda c: c["name"])
API = types.SimpleNamespace(make_snowpack=make_snowpack, make_soil=make_soil, make_interface=make_interface,
                            lrm_altimeter_list=lrm_altimeter_list)


def golden(case):
    return np.load(os.path.join(GOLDEN, "nadir_lrm_altimetry_" + case["name"] + ".npz"))


_RESTATED = {}


def restated(case):
    """The restatement of a case, computed once and shared (never modified)."""
    if case["name"] not in _RESTATED:
        _RESTATED[case["name"]] = solve_case(case, API)
    return _RESTATED[case["name"]]


def assert_waveform(values, reference, what):
    peak = float(np.abs(reference[-1]).max())
    err = float(np.abs(values - reference).max())
    print(f"{what}: largest difference {err:.3e}, peak of the total {peak:.3e}, ratio {err / peak if peak else 0.0:.3e} (bar {REL_BAR:g})")
    assert values.shape == reference.shape and np.all(np.isfinite(values)) and err <= REL_BAR * peak, (what, err, peak)


def assert_close(a, b, rtol, what, to_max=False):
    """Element by element relative to the reference's element; to_max: relative to the largest |element| of the reference (an
    axis with an exact zero on it, such as delay at the nominal gate)."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), what
    ok = ~np.isnan(b)
    if to_max:
        err = float(np.abs(a[ok] - b[ok]).max() / np.abs(b[ok]).max())
        print(f"{what}: largest difference relative to the largest value {err:.3e} (bar {rtol:g})")
        assert err <= rtol, (what, err)
        return
    err = float((np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1e-300)).max()) if ok.any() and np.abs(b[ok]).max() > 0 else float(np.abs(a[ok]).max(initial=0.0))
    print(f"{what}: largest relative difference {err:.3e} (bar {rtol:g})")
    assert err <= rtol, (what, err)


def assert_scalars(eps, ke, bs, g, what):
    assert_close(eps, g["eps"], 1e-12, what + " eps")
    assert_close(ke, g["ke"], 1e-10, what + " ke")
    assert_close(bs, g["backward_scattering"], 1e-10, what + " backward scattering")


def assert_vertical(vertical, g, what):
    """The vertical distribution before the convolution, on the sub-gates both have; the bar is that of the waveform, against the
    largest entry of the fixture's distribution."""
    ref = g["vertical"]
    n = min(vertical.shape[1], ref.shape[1])
    scale = float(np.abs(ref).max())
    err = float(np.abs(vertical[:, :n] - ref[:, :n]).max())
    print(f"{what} vertical distribution: largest difference {err:.3e}, largest entry {scale:.3e}")
    assert vertical.shape[0] == ref.shape[0] and err <= REL_BAR * scale and np.all(vertical[:, n:] == 0.0)


# ---- restatement against the fixtures -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, **IDS)
def test_restatement_reproduces_the_fixture(case):
    g, sol = golden(case), restated(case)
    assert_waveform(sol["waveform"], g["waveform"], "restatement " + case["name"])
    assert_scalars(sol["eps"], sol["ke"], sol["backward_scattering"], g, "restatement " + case["name"])
    assert_vertical(sol["vertical"], g, "restatement " + case["name"])
    for name in ("z_gate", "delay", "gate"):
        assert_close(sol[name], g[name], 1e-12, name, to_max=name == "delay")


def test_fixtures_cover_what_they_must():
    gs = {c["name"]: golden(c) for c in CASES}
    assert np.all(gs["nonscattering"]["waveform"] == 0.0)                      # no scattering, Flat interfaces: exactly nothing
    assert gs["deep"]["vertical"].shape[1] > 16 * 10                           # more sub-gates than the window has
    assert gs["shallow"]["vertical"].shape[1] == 2                             # shallower than one sub-gate
    assert gs["os3_ng8"]["vertical"].shape[0] == 1 and 3 * 8 < 64 < 5 * 13     # below and just above one wavefront
    assert gs["rough_tis8_contrib"]["waveform"].shape == (4, 16) and gs["oversampled"]["waveform"].shape == (1, 160)
    assert gs["envisat_ku"]["waveform"].shape == (1, 128)
    assert np.isnan(gs["flat_L1"]["z_gate"]).any() and not np.isnan(gs["deep"]["z_gate"]).any()
    assert np.count_nonzero(np.diff(np.searchsorted(np.cumsum(case_by_name("thin_layers")["thickness"]), gs["thin_layers"]["z_gate"][:2])) > 3)


# ---- the device source on the CPU ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_lib():
    lib = host_library("libsmrt_lrm_host.so", "nadir_lrm_altimetry_host.cpp")
    lib.smrt_lrm_host_run.restype = C.c_int32
    lib.smrt_lrm_host_layers.restype = C.c_int32
    lib.smrt_lrm_host_i0.restype = C.c_double
    lib.smrt_lrm_host_i0.argtypes = [C.c_double]
    return lib


class HostContext:
    """Stands in for DortContext: the same call, answered by the CPU build of the device source."""

    def __init__(self, lib):
        self.lib, self.lock, self.calls = lib, threading.RLock(), 0

    def lrm_run(self, batch, params, pairs=None):
        self.calls += 1
        o = _native.LrmOutput(batch, params, batch.n_pairs)
        assert self.lib.smrt_lrm_host_run(C.byref(batch.struct), C.byref(params.struct), *o.pointers()) == 0
        if pairs is not None:
            for name in ("values", "status", "z_gate", "layers", "vertical"):
                setattr(o, name, getattr(o, name)[np.asarray(pairs)])
        self.last = o
        return o

    def lrm_layers(self, batch, params):
        a = np.empty((batch.n_pairs, int(batch.struct.n_layers_max), 5))
        assert self.lib.smrt_lrm_host_layers(C.byref(batch.struct), a.ctypes.data_as(C.POINTER(C.c_double))) == 0
        return a


@pytest.fixture()
def on_host(host_lib, monkeypatch):
    from smrt_amd.rtsolver import nadir_lrm_altimetry as module

    ctx = HostContext(host_lib)
    monkeypatch.setattr(module, "get_context", lambda device=None: ctx)
    return ctx


def run_case(case):
    m = make_model(case.get("emmodel", "iba"), "nadir_lrm_altimetry", rtsolver_options=solver_options(case))
    return m, m.run(make_sensor(case, API), build_snowpack(case, API))


def waveform_of(res):
    w = res.data.values[..., 0, 0]
    return w if w.ndim == 2 else w[None]


@pytest.mark.parametrize("case", CASES, **IDS)
def test_device_source_on_the_cpu_through_model_run_reproduces_the_fixture_and_the_restatement(on_host, case):
    g = golden(case)
    m, res = run_case(case)
    assert isinstance(res, AltimetryResult)
    contributions = solver_options(case).get("return_contributions", False)
    assert res.data.dims == (("contribution",) if contributions else ()) + ("delay", "theta_inc", "theta")
    if contributions:
        assert list(res.contributions()) == ["surface", "interfaces", "volume", "total"]
    assert_waveform(waveform_of(res), g["waveform"], "device source on the CPU " + case["name"])
    assert_waveform(waveform_of(res), restated(case)["waveform"], "device source against the restatement " + case["name"])
    assert_close(res.delay, g["delay"], 1e-12, "delay", to_max=True)
    assert_close(res.gate, g["gate"], 1e-12, "gate")
    assert_close(res.z_gate.values, g["z_gate"], 1e-12, "z_gate")
    other = res.other_data
    assert_scalars(other["effective_permittivity"].values.real, other["ke"].values, other["backward_scattering"].values, g, case["name"])
    assert_vertical(on_host.last.vertical[0], g, "device source on the CPU " + case["name"])
    total = res.waveform()
    assert np.allclose(np.ravel(total), 4 * np.pi * g["waveform"][-1], rtol=1e-6, atol=0)


@pytest.mark.parametrize("name", ["rough_tis4", "rough_fast_coherent", "shallow"])
def test_rough_interfaces_and_a_substrate_still_cost_one_launch(on_host, name):
    """The permittivities the host evaluation needs come from the (pair, layer) kernel alone, not from a launch of the solver."""
    from smrt_amd.rtsolver.nadir_lrm_altimetry import NadirLRMAltimetry

    case = case_by_name(name)
    m = make_model("iba", "nadir_lrm_altimetry", rtsolver_options=solver_options(case))
    solver = NadirLRMAltimetry(**solver_options(case))
    sps = [build_snowpack(case, API) for _ in range(3)]
    res = solver.solve_plan(m, m.plan(make_sensor(case, API), sps))
    assert solver.launches == 1 and on_host.calls == 1 and res.data.shape[0] == 3
    assert_waveform(res.data.values[2, :, 0, 0][None], golden(case)["waveform"], "batch of three " + name)


def test_bessel_i0_against_scipy(host_lib):
    from scipy.special import i0

    x = np.concatenate([np.linspace(0.0, 20.0, 401), np.linspace(20.0, 700.0, 400), [1e-9, 19.999, 20.001, -3.0]])
    mine = np.array([host_lib.smrt_lrm_host_i0(float(v)) for v in x])
    err = np.abs(mine / i0(x) - 1.0).max()
    print(f"I0: largest relative difference from scipy.special.i0 {err:.3e}")
    assert err < 5e-14


def test_sensor_list_against_the_reference():
    g = np.load(os.path.join(GOLDEN, "lrm_altimeter_list.npz"))
    names = [str(n) for n in g["names"]]
    sensors = {"envisat_ra2": lrm_altimeter_list.envisat_ra2(), "sentinel3_sral": lrm_altimeter_list.sentinel3_sral(),
               "saral_altika": lrm_altimeter_list.saral_altika(), "cryosat2_lrm": lrm_altimeter_list.cryosat2_lrm(),
               "asiras_lam": lrm_altimeter_list.asiras_lam(altitude=1000.0),
               "envisat_ra2_tilted": lrm_altimeter_list.envisat_ra2("Ku", pitch_angle_deg=0.1, roll_angle_deg=0.2)}
    seen = set()
    for key, s in sensors.items():
        for one in (s.sensor_list if hasattr(s, "sensor_list") else [s]):
            channel = list(one.channel_map)[0]
            mine = np.array([float(np.ravel(getattr(one, n))[0]) for n in names])
            assert np.array_equal(mine, g[f"{key}.{channel}"]), (key, channel, dict(zip(names, mine - g[f"{key}.{channel}"])))
            seen.add(f"{key}.{channel}")
    assert seen == set(g.files) - {"names"}
    assert lrm_altimeter_list.envisat_ra2("Ku").mode == "A"
    with pytest.raises(SMRTError, match="altitude"):
        lrm_altimeter_list.asiras_lam()


# ---- the Python layer -------------------------------------------------------------------------------------------------------
def test_plugin_resolution_and_options():
    from smrt_amd.core.plugin import import_class
    from smrt_amd.rtsolver.lrm_waveform_model import Brown1977
    from smrt_amd.rtsolver.nadir_lrm_altimetry import NadirLRMAltimetry

    assert import_class("rtsolver", "nadir_lrm_altimetry") is NadirLRMAltimetry
    d = NadirLRMAltimetry()
    assert (d.oversampling, d.return_oversampled, d.skip_pfs_convolution, d.return_contributions, d.compute_coherent_reflection,
            d.theta_inc_sampling, d.error_handling, d.launches) == (10, False, False, False, True, 8, "exception", 0)
    assert NadirLRMAltimetry(waveform_model=Brown1977).theta_inc_sampling == 8
    Newkrik1992 = type("Newkrik1992", (), {})
    for bad in (dict(waveform_model=Newkrik1992), dict(error_handling="ignore"), dict(oversampling_time=0), dict(theta_inc_sampling=0),
                dict(skip_pfs_convolution=True), dict(skip_pfs_convolution=True, theta_inc_sampling=4)):
        with pytest.raises(SMRTError):
            NadirLRMAltimetry(**bad)
    assert NadirLRMAltimetry(skip_pfs_convolution=True, theta_inc_sampling=1).skip_pfs_convolution


def test_what_the_reference_cannot_run_is_refused(on_host):
    from smrt_amd.atmosphere.simple_isotropic_atmosphere import SimpleIsotropicAtmosphere
    from smrt_amd import sensor_list

    kw = dict(density=[300.0, 350.0], temperature=[260.0, 260.0], corr_length=[2e-4, 2e-4])
    flat = make_snowpack([1.0, 2.0], "exponential", **kw)
    sensor = lrm_altimeter_list.lrm_altimeter(channel="Ku", **SMALL)
    fast = make_model("iba", "nadir_lrm_altimetry", rtsolver_options=dict(theta_inc_sampling=1))
    slow = make_model("iba", "nadir_lrm_altimetry")
    with pytest.raises(SMRTError, match="nadir looking altimeter only"):
        slow.run(lrm_altimeter_list.lrm_altimeter(channel="Ku", theta_inc_deg=2.0, **SMALL), flat)
    with pytest.raises(SMRTError, match="altimeter sensor"):
        slow.run(sensor_list.active(13e9, 0), flat)
    with pytest.raises(SMRTError, match="atmosphere"):
        slow.run(sensor, SimpleIsotropicAtmosphere(tb_down=20.0, tb_up=18.0, transmittance=0.9) + flat)
    with pytest.raises(SMRTError, match="true divider"):
        make_model("iba", "nadir_lrm_altimetry", rtsolver_options=dict(theta_inc_sampling=5)).run(sensor, flat)
    rough_sea = make_snowpack([1.0, 2.0], "exponential", **kw)
    rough_sea.sigma_surface = 0.2
    with pytest.raises(SMRTError, match="sigma_surface"):
        slow.run(sensor, rough_sea)
    assert np.all(np.isfinite(fast.run(sensor, rough_sea).data.values))
    gob = make_snowpack([1.0, 2.0], "exponential", interface=[make_interface("geometrical_optics_backscatter", mean_square_slope=0.03)] * 2, **kw)
    with pytest.raises(SMRTError, match="roughness_rms"):
        slow.run(sensor, gob)
    assert np.all(np.isfinite(make_model("iba", "nadir_lrm_altimetry", rtsolver_options=dict(compute_coherent_reflection=False))
                              .run(sensor, gob).data.values))
    mixed = make_snowpack([1.0, 2.0], "exponential", interface=[make_interface("iem_fung92", roughness_rms=5e-4, corr_length=1e-2), None], **kw)
    with pytest.raises(SMRTError, match="all have a roughness_rms or all have none"):
        fast.run(sensor, mixed)
    assert np.all(np.isfinite(slow.run(sensor, mixed).data.values))
    for nominal_gate in (0, 16, 40):     # no sub-gate at or after it, or the first one: the reference's shift fails
        with pytest.raises(SMRTError, match="nominal gate must lie inside the gate window"):
            fast.run(lrm_altimeter_list.lrm_altimeter(channel="Ku", **dict(SMALL, nominal_gate=nominal_gate)), flat)
    assert np.all(np.isfinite(slow.run(lrm_altimeter_list.lrm_altimeter(channel="Ku", **dict(SMALL, nominal_gate=0)), flat).data.values))
    tilted = make_snowpack([1.0, 2.0], "exponential", **kw)
    tilted.surface_slope = 0.1
    with pytest.raises(SMRTError, match="both off_nadir and tilted terrain"):
        fast.run(lrm_altimeter_list.lrm_altimeter(channel="Ku", pitch_angle_deg=0.1, **SMALL), tilted)


def test_batches_groups_error_handling_and_files(on_host, tmp_path):
    kw = dict(corr_length=2e-4)
    sps = [make_snowpack([0.5, 1.0 + k, 2.0][:1 + k % 3], "exponential", density=[300.0, 350.0, 400.0][:1 + k % 3],
                         temperature=[258.0, 260.0, 262.0][:1 + k % 3], **kw) for k in range(5)]
    m = make_model("iba", "nadir_lrm_altimetry", rtsolver_options=dict(return_contributions=True))
    two = lrm_altimeter_list.make_multi_channel_altimeter({"narrow": SMALL, "wide": dict(SMALL, beamwidth_alongtrack=5.5, frequency=3.2e9)}, None)
    res = m.run(two, sps)    # two sensor configurations: two groups, one launch each
    assert on_host.calls == 2 and res.data.dims == ("channel", "snowpack", "contribution", "delay", "theta_inc", "theta")
    assert res.data.shape == (2, 5, 4, 16, 1, 1) and res.z_gate.shape == (2, 5, 16) and list(res.data.coords["channel"]) == ["narrow", "wide"]
    one = lrm_altimeter_list.lrm_altimeter(channel="Ku", **SMALL)
    both = m.run(one, sps)
    assert on_host.calls == 3 and both.data.dims == ("snowpack", "contribution", "delay", "theta_inc", "theta")
    single = m.run(one, sps[3])
    assert np.array_equal(single.data.values, both.data.values[3]) and np.array_equal(single.z_gate.values, both.z_gate.values[3], equal_nan=True)
    assert np.array_equal(np.ravel(both.waveform(contribution="volume", snowpack=3)), 4 * np.pi * single.data.values[2, :, 0, 0])
    # error handling: one element marked, its neighbours intact
    warm = make_snowpack([0.5, 2.0], "exponential", density=[300.0, 320.0], temperature=[260.0, 280.0], **kw)
    with pytest.raises(SMRTError, match="Invalid layer properties"):
        m.run(one, [sps[0], warm, sps[1]])
    nan = make_model("iba", "nadir_lrm_altimetry", rtsolver_options=dict(return_contributions=True, error_handling="nan"))
    marked = nan.run(one, [sps[0], warm, sps[1]])
    assert np.all(np.isnan(marked.data.values[1])) and np.array_equal(marked.data.values[[0, 2]], both.data.values[[0, 1]])
    # files
    path = str(tmp_path / "waveform.nc")
    both.save(path)
    back = open_result(path)
    assert isinstance(back, AltimetryResult) and back.data.dims == both.data.dims and np.array_equal(back.data.values, both.data.values)
    assert np.array_equal(back.z_gate.values, both.z_gate.values, equal_nan=True) and np.allclose(back.gate, both.gate, rtol=1e-15)
    assert list(back.contributions()) == ["surface", "interfaces", "volume", "total"]


def test_header_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "smrt_dort.h")).read()
    body = header[header.index("typedef struct smrt_lrm_params {"):header.index("} smrt_lrm_params;")]
    declared = [line.split(";")[0].split()[-1].lstrip("*") for line in body.splitlines()[1:] if ";" in line]
    assert declared == [name for name, _ in _native.LrmParams._fields_]
    lib = _native.load_library()
    for name in ("out_stride", "run_pairs", "upload_pairs", "launch", "sync", "layers", "download", "kernel_ms", "abi"):
        assert "smrt_lrm_" + name in _native.EXPORTED_SYMBOLS and hasattr(lib, "smrt_lrm_" + name) and ("smrt_lrm_" + name + "(") in header
    assert _native.lrm_params_layout() == _native.lrm_abi_layout(lib)
