"""The nadir SAR altimetry solver without a GPU: the NumPy / SciPy restatement against every fixture, the DEVICE arithmetic
(smrt_amd/csrc/nadir_sar_altimetry_kernel.hpp) compiled with g++ against every fixture and against the restatement, f0 and f1 of
the device against scipy.special.ive, the sensor list against its fixture, the refusals, and the Python layer (plugin, options,
dims, coords, error handling, save / open_result) driven end to end with the CPU build of the kernels in place of the GPU context.

Bars: every sample of every contribution within 1e-8 x the largest value of the case's total map; z_gate, delay, gate, Doppler
frequency and Doppler bin 1e-12 relative; f0 and f1 1e-10 absolute.  Measured: profiles/nadir_sar_altimetry_parity.txt."""
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
from smrt_amd.core.terrain import TerrainInfo
from smrt_amd.inputs import sar_altimeter_list
from smrt_amd.inputs.make_medium import make_interface, make_snowpack, make_soil
from nadir_sar_altimetry_restatement import (CASES, REL_BAR, build_snowpack, case_by_name, contribution_names, make_sensor, solve_case,
                                             solver_options, surface_map)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
IDS = dict(ids=lambda c: c["name"])
API = types.SimpleNamespace(make_snowpack=make_snowpack, make_soil=make_soil, make_interface=make_interface,
                            sar_altimeter_list=sar_altimeter_list, TerrainInfo=TerrainInfo)
_GO = dict(roughness_rms=0.005, corr_length=0.10)
SMRT_ERR_INPUT = 5     # include/smrt_dort.h


def golden(case):
    return np.load(os.path.join(GOLDEN, "nadir_sar_altimetry_" + case["name"] + ".npz"))


_RESTATED = {}


def restated(case):
    """The restatement of a case, computed once and shared (never modified)."""
    if case["name"] not in _RESTATED:
        _RESTATED[case["name"]] = solve_case(case, API)
    return _RESTATED[case["name"]]


def assert_map(values, reference, what):
    peak = float(np.abs(reference[-1]).max())
    assert values.shape == reference.shape, (what, values.shape, reference.shape)
    err = float(np.abs(values - reference).max())
    print(f"{what}: largest difference {err:.3e}, largest value of the total {peak:.3e}, ratio to the bar {err / peak / REL_BAR:.3e}")
    assert np.all(np.isfinite(values)) and err <= REL_BAR * peak, (what, err, peak)


def assert_close(a, b, rtol, what):
    """Relative to the largest |element| of the reference (the axes have a zero, or nearly one, on them)."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), what
    ok = ~np.isnan(b)
    err = float(np.abs(a[ok] - b[ok]).max() / np.abs(b[ok]).max())
    print(f"{what}: largest difference relative to the largest value {err:.3e} (bar {rtol:g})")
    assert err <= rtol, (what, err)


def assert_z_gate(a, b, what):
    """Element by element (the first gate is 1e-25 m by definition)."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), what
    ok = ~np.isnan(b)
    err = float((np.abs(a[ok] - b[ok]) / np.abs(b[ok])).max())
    print(f"{what}: largest relative difference {err:.3e} (bar 1e-12)")
    assert err <= 1e-12, (what, err)


def assert_axes(sol, g, what):
    for name in ("delay", "doppler_frequency", "gate", "doppler_bin"):
        assert_close(sol[name], g[name], 1e-12, what + " " + name)
    assert_z_gate(sol["z_gate"], g["z_gate"], what + " z_gate")


def assert_vertical(vertical, echo, g, what):
    """The volume backscatter on the sub-gates both have, and the echo of the boundaries; the bar is that of the map, against the
    largest entry of the fixture's."""
    ref = g["vertical"]
    n = min(len(vertical), len(ref))
    scale = float(np.abs(ref).max())
    err = float(np.abs(vertical[:n] - ref[:n]).max())
    print(f"{what} volume backscatter: largest difference {err:.3e}, largest entry {scale:.3e}")
    assert err <= REL_BAR * scale and np.all(vertical[n:] == 0.0)
    scale = float(np.abs(g["echo"]).max())
    err = float(np.abs(echo - g["echo"]).max())
    print(f"{what} echo of the boundaries: largest difference {err:.3e}, largest entry {scale:.3e}")
    assert err <= REL_BAR * scale


# ---- restatement against the fixtures -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, **IDS)
def test_restatement_reproduces_the_fixture(case):
    g, sol = golden(case), restated(case)
    assert list(g["contributions"]) == sol["contributions"]
    assert_map(sol["ddm"], g["ddm"], "restatement " + case["name"])
    assert_axes(sol, g, "restatement " + case["name"])
    assert_vertical(sol["vertical"], sol["echo"], g, "restatement " + case["name"])
    assert_close(sol["t_interface"], g["t_interface"], 1e-12, "t_interface")


def test_fixtures_cover_what_they_must():
    gs = {c["name"]: golden(c) for c in CASES}
    sizes = {(len(g["vertical"]), g["ddm"].shape) for g in gs.values()}
    assert len(sizes) > 5
    assert gs["n63_d60_basic"]["ddm"].shape == (4, 63, 20) and gs["n65_d68_full_oversampled"]["ddm"].shape == (3, 65, 68)
    assert gs["n64_d64_basic_coherent"]["ddm"].shape == (6, 16, 16) and gs["cryosat2_sarm"]["ddm"].shape == (1, 128, 64)
    assert len(gs["deep_pruned"]["vertical"]) > 64 and len(gs["deep_pruned"]["t_interface"]) == 4      # four layers, three kept
    assert len(gs["shallow_substrate"]["vertical"]) < 32 and np.isnan(gs["shallow_substrate"]["z_gate"]).any()
    assert restated(case_by_name("last_sample"))["shift"][1] == 31
    coherent = gs["n64_d64_basic_coherent"]["ddm"]
    assert coherent[1].max() > 1e-3 * coherent[-1].max()                                                 # the coherent surface echo counts
    rough = gs["n65_d68_full_oversampled"]["echo"]
    assert 0 < rough[0, 0] < 1e-20 * rough[1, 0]                                                         # ... and here it does not
    assert gs["pitch_roll_full_coherent"]["ddm"].shape[0] == 2 * 4 + 2 and gs["last_sample"]["ddm"].shape[0] == 2 + 2


# ---- the device source on the CPU ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_lib():
    lib = host_library("libsmrt_sar_host.so", "nadir_sar_altimetry_host.cpp")
    lib.smrt_sar_host_run.restype = C.c_int32
    lib.smrt_sar_host_refusal.restype = C.c_char_p
    for f in (lib.smrt_sar_host_f0, lib.smrt_sar_host_f1):
        f.restype, f.argtypes = C.c_double, [C.c_double]
    lib.layers = host_library("libsmrt_lrm_host.so", "nadir_lrm_altimetry_host.cpp")
    lib.layers.smrt_lrm_host_layers.restype = C.c_int32
    return lib


class HostContext:
    """Stands in for DortContext: the same calls, answered by the CPU build of the device source."""

    def __init__(self, lib):
        self.lib, self.lock, self.calls = lib, threading.RLock(), 0

    def sar_run(self, batch, params, pairs=None):
        self.calls += 1
        o = _native.SarOutput(batch, params, batch.n_pairs)
        assert self.lib.smrt_sar_host_run(C.byref(batch.struct), C.byref(params.struct), *o.pointers()) == 0
        if pairs is not None:
            for name in ("values", "status", "z_gate", "layers", "vertical", "echo"):
                setattr(o, name, getattr(o, name)[np.asarray(pairs)])
        self.last, self.last_params, self.batch = o, params, batch
        return o

    def lrm_layers(self, batch, params):
        a = np.empty((batch.n_pairs, int(batch.struct.n_layers_max), 5))
        assert self.lib.layers.smrt_lrm_host_layers(C.byref(batch.struct), a.ctypes.data_as(C.POINTER(C.c_double))) == 0
        return a


@pytest.fixture()
def on_host(host_lib, monkeypatch):
    from smrt_amd.rtsolver import nadir_sar_altimetry as module

    ctx = HostContext(host_lib)
    monkeypatch.setattr(module, "get_context", lambda device=None: ctx)
    return ctx


def run_case(case):
    m = make_model("iba", "nadir_sar_altimetry", rtsolver_options=solver_options(case))
    return m, m.run(make_sensor(case, API), build_snowpack(case, API))


def map_of(res):
    w = res.data.values[..., 0, 0]
    return w if w.ndim == 3 else w[None]


@pytest.mark.parametrize("case", CASES, **IDS)
def test_device_source_on_the_cpu_through_model_run_reproduces_the_fixture_and_the_restatement(on_host, case):
    g = golden(case)
    m, res = run_case(case)
    assert isinstance(res, AltimetryResult)
    names = list(g["contributions"])
    assert res.data.dims == (("contribution",) if names else ()) + ("delay", "doppler_frequency", "theta_inc", "theta")
    if names:
        assert list(res.contributions()) == names
    assert_map(map_of(res), g["ddm"], "device source on the CPU " + case["name"])
    assert_map(map_of(res), restated(case)["ddm"], "device source against the restatement " + case["name"])
    mine = dict(delay=res.delay, doppler_frequency=res.doppler_frequency, gate=res.gate, doppler_bin=res.doppler_bin, z_gate=res.z_gate.values)
    assert_axes(mine, g, "device source on the CPU " + case["name"])
    o = on_host.last
    nb = g["echo"].shape[1]
    assert_vertical(o.vertical[0], o.echo[0, :nb, 1:3].T, g, "device source on the CPU " + case["name"])
    assert_close(o.echo[0, :nb, 0], g["t_interface"], 1e-12, "t_interface")
    assert np.array_equal(o.echo[0, :nb, 3], restated(case)["shift"])
    total = res.waveform()
    assert np.allclose(np.ravel(total), 4 * np.pi * g["ddm"][-1].sum(axis=1), rtol=0, atol=4 * np.pi * REL_BAR * g["ddm"][-1].sum(axis=1).max())
    # The coefficient of f1 in D18 eq. 22 next to f0's, which is 1, at its largest (the nu of the coherent echo, gl at nadir): an
    # error of 1e-10 in f1 weighs coefficient x 1e-10 in the map, so the bar of f1 holds the map's 1e-8 as long as it is below 100.
    p = on_host.last_params.struct
    sigma = case.get("sigma_surface", 0.0)
    coefficient = sigma / p.l_gamma * (1 + p.nu_coherent / p.gamma_y) / (p.pulse_bandwidth * p.sigma_p) * sigma / p.lz
    print(f"{case['name']}: coefficient of f1 at most {coefficient:.3e} (f0's is 1)")
    assert coefficient < 1e2


def test_bessel_combinations_against_scipy(host_lib):
    from nadir_sar_altimetry_restatement import f0, f1
    cross = 2 * np.sqrt(30.0)     # kSarCrossover: x = xi^2 / 4 = 30
    xi = np.concatenate([np.linspace(-160.0, 160.0, 3201), [0.0, 1e-12, -1e-12, 1e-9, -1e-9, 2e-10, 1.9e-10],
                         cross * np.array([1 - 1e-9, 1.0, 1 + 1e-9, -1 + 1e-9, -1.0, -1 - 1e-9]), np.linspace(cross - 0.5, cross + 0.5, 101)])
    mine0 = np.array([host_lib.smrt_sar_host_f0(float(v)) for v in xi])
    mine1 = np.array([host_lib.smrt_sar_host_f1(float(v)) for v in xi])
    # Below x = xi^2 / 4 = 1e-20 the device returns the reference's limits (D18 eq. 11, 12), as the reference does: the value to
    # hold it to there is the limit itself, f(0) (the function has moved from it by up to |f1'(0)| x 2e-10 = 1.1e-10 at the edge).
    masked = xi ** 2 / 4 < 1e-20
    want0, want1 = np.where(masked, f0(np.zeros(1)), f0(xi)), np.where(masked, f1(np.zeros(1)), f1(xi))
    e0, e1 = np.abs(mine0 - want0).max(), np.abs(mine1 - want1).max()
    print(f"f0: largest difference from scipy.special.ive {e0:.3e}; f1: {e1:.3e} (bar 1e-10, absolute)")
    assert e0 <= 1e-10 and e1 <= 1e-10
    assert np.abs(mine0).max() < 3 and np.abs(mine1).max() < 3     # both O(1)


def test_sensor_list_against_the_reference():
    import importlib.util

    g = np.load(os.path.join(GOLDEN, "sar_altimeter_list.npz"))
    spec = importlib.util.spec_from_file_location("sar_fixture_maker_names", os.path.join(GOLDEN, "make_nadir_sar_altimetry_fixtures.py"))
    source = open(spec.origin).read()
    names = [str(n) for n in g["names"]]
    assert all(f'"{n}"' in source for n in names)
    sensors = {"cryosat2_sarm": sar_altimeter_list.cryosat2_sarm(), "cryosat2_sarm_circular_tilted": sar_altimeter_list.cryosat2_sarm(0.1, 0.2, True),
               "sentinel3_sarm_Ku_ocean": sar_altimeter_list.sentinel3_sarm("Ku", "ocean"),
               "sentinel3_sarm_C_landice": sar_altimeter_list.sentinel3_sarm("C", "landice"),
               "sentinel3_sarm_C_seaice": sar_altimeter_list.sentinel3_sarm("C", "seaice"), "cristal_Ku": sar_altimeter_list.cristal("Ku"),
               "cristal_Ka_circular": sar_altimeter_list.cristal("Ka", force_circular_antenna=True)}
    for key, one in sensors.items():
        mine = np.array([float(np.ravel(getattr(one, n))[0]) for n in names])
        assert np.array_equal(mine, g[key]), (key, dict(zip(names, mine - g[key])))
        assert [one.doppler_window, list(one.channel_map)[0]] == list(g[key + ".window_channel"])
    assert set(g.files) == {"names"} | set(sensors) | {k + ".window_channel" for k in sensors}
    for bad in (lambda: sar_altimeter_list.sentinel3_sarm("Ku", "lake"), lambda: sar_altimeter_list.sentinel3_sarm("S", "ocean"),
                lambda: sar_altimeter_list.cristal("C")):
        with pytest.raises(SMRTError):
            bad()


# ---- the Python layer -------------------------------------------------------------------------------------------------------
def test_plugin_resolution_and_options():
    from smrt_amd.core.plugin import import_class
    from smrt_amd.rtsolver.nadir_sar_altimetry import Dinardo18, NadirSARAltimetry

    assert import_class("rtsolver", "nadir_sar_altimetry") is NadirSARAltimetry
    d = NadirSARAltimetry()
    assert (d.oversampling_time, d.oversampling_doppler, d.return_oversampled, d.return_contributions, d.return_coherent,
            d.prune_deep_snowpack, d.error_handling, d.launches, d.ptr_doppler) == (4, 4, False, "no", False, True, "exception", 0, "gaussian-smrt")
    assert NadirSARAltimetry(delay_doppler_model="dinardo18").return_contributions == "no"
    assert NadirSARAltimetry(delay_doppler_model=Dinardo18, return_contributions="full coherent").return_coherent
    Ray15 = type("Ray15", (), {})
    for bad in (dict(delay_doppler_model="ray15"), dict(delay_doppler_model=Ray15), dict(delay_doppler_model="landy19"),
                dict(delay_doppler_model=3)):
        with pytest.raises(SMRTError, match="Dinardo18"):
            NadirSARAltimetry(**bad)
    for bad in (dict(error_handling="ignore"), dict(oversampling_time=0), dict(oversampling_doppler=1.5), dict(skip_convolutions=True),
                dict(return_contributions="everything"), dict(delay_doppler_model_options=dict(grid_space=300)),
                dict(delay_doppler_model_options=dict(ptr_time="sinc^2"))):
        with pytest.raises(SMRTError):
            NadirSARAltimetry(**bad)


def reduced(**kwargs):
    return make_sensor(dict(sensor=dict(ngate=8, nominal_gate=3, ndoppler=4, **kwargs)), API)


def snowpack(thickness=(1.0,), interface=None, substrate=None, terrain_info="default", **kw):
    n = len(thickness)
    itf = [make_interface("geometrical_optics_backscatter", **_GO) for _ in range(n)] if interface is None else interface
    sp = make_snowpack(list(thickness), "exponential", density=[300.0, 350.0, 400.0][:n], temperature=[258.0, 260.0, 262.0][:n],
                       corr_length=2e-4, interface=itf, substrate=substrate, **kw)
    sp.terrain_info = TerrainInfo(sigma_surface=0.2) if terrain_info == "default" else terrain_info
    return sp


def test_what_the_reference_cannot_run_is_refused(on_host):
    from smrt_amd import sensor_list
    from smrt_amd.atmosphere.simple_isotropic_atmosphere import SimpleIsotropicAtmosphere

    m = make_model("iba", "nadir_sar_altimetry")
    sensor = reduced()
    assert np.all(np.isfinite(m.run(sensor, snowpack()).data.values))
    tilted = sar_altimeter_list.sar_altimeter(channel="Ku", frequency=13.575e9, altitude=717e3, pulse_bandwidth=320e6, beamwidth_alongtrack=1.1,
                                              beamwidth_acrosstrack=1.1, pulse_repetition_frequency=17825, velocity=7435, ngate=8, ndoppler=4,
                                              nominal_gate=3, doppler_window="hamming", theta_inc_deg=2.0)
    with pytest.raises(SMRTError, match="nadir looking altimeter only"):
        m.run(tilted, snowpack())
    with pytest.raises(SMRTError, match="SAR altimeter sensor"):
        m.run(sensor_list.active(13e9, 0), snowpack())
    with pytest.raises(SMRTError, match="atmosphere"):
        m.run(sensor, SimpleIsotropicAtmosphere(tb_down=20.0, tb_up=18.0, transmittance=0.9) + snowpack())
    odd = reduced()
    odd.ndoppler = 5
    with pytest.raises(SMRTError, match="even"):
        m.run(odd, snowpack())
    for interface in ([None], [make_interface("transparent")]):     # Flat and Transparent have no roughness_rms
        with pytest.raises(SMRTError, match="roughness_rms"):
            m.run(sensor, snowpack(interface=interface))
    with pytest.raises(SMRTError, match="roughness_rms"):
        m.run(sensor, snowpack(substrate=make_soil("flat", complex(5.0, 0.5), temperature=270.0)))
    with pytest.raises(SMRTError, match="roughness_rms"):
        m.run(sensor, snowpack(interface=[make_interface("geometrical_optics_backscatter", mean_square_slope=0.01)]))
    with pytest.raises(SMRTError, match="mean_square_slope"):
        m.run(sensor, snowpack(interface=[make_interface("iem_fung92", roughness_rms=5e-4, corr_length=1e-2)]))
    with pytest.raises(SMRTError, match="normally-distributed"):
        m.run(sensor, snowpack(terrain_info=TerrainInfo(distribution="lognormal", sigma_surface=0.2)))
    # of smrt_amd's own
    assert np.all(np.isfinite(m.run(sensor, snowpack(terrain_info=None)).data.values))
    with pytest.raises(SMRTError, match="dem"):
        m.run(sensor, snowpack(terrain_info=TerrainInfo(dem=np.zeros((2, 2)))))
    with pytest.raises(SMRTError, match="slope_angle"):
        m.run(sensor, snowpack(terrain_info=TerrainInfo(slope_angle=0.01)))
    # a boundary with a positive echo later than the window (8 x 4 sub-gates): the reference's `assert 0 <= itime < N`
    late = snowpack(thickness=(3.4, 1.0))     # (above the depth the pruning cuts at, 3.75 m, and slower than in vacuum)
    with pytest.raises(SMRTError, match="later than the window"):
        m.run(sensor, late)
    nan = make_model("iba", "nadir_sar_altimetry", rtsolver_options=dict(error_handling="nan"))
    marked = nan.run(sensor, [snowpack(), late])
    assert np.all(np.isnan(marked.data.values[1])) and np.all(np.isfinite(marked.data.values[0])) and list(on_host.last.status) == [0, SMRT_ERR_INPUT]


def test_c_abi_refusals(host_lib, on_host):
    """What smrt_sar_upload_pairs answers before any device work (smrt_amd/csrc/solver_refusals.hpp)."""
    make_model("iba", "nadir_sar_altimetry").run(reduced(), snowpack())
    batch_params = on_host.last_params

    def refusal(**changes):
        p = _native.SarParams.from_buffer_copy(batch_params.struct)
        for k, v in changes.items():
            setattr(p, k, v)
        return host_lib.smrt_sar_host_refusal(C.byref(on_host.batch.struct), C.byref(p))

    # (the batch of the last run, kept by the context below)
    assert refusal() is None
    assert b"even" in refusal(ndoppler=5) and b"positive" in refusal(oversampling_doppler=0) and b"invalid sensor" in refusal(velocity=0.0)
    assert b"n_rows" in refusal(n_rows=0) and b"missing" in refusal(n_tables=0)


def test_batches_groups_error_handling_and_files(on_host, tmp_path):
    sps = [snowpack(thickness=(0.5, 0.4 + 0.1 * k, 0.5)[:1 + k % 3]) for k in range(5)]
    for k, sp in enumerate(sps):
        sp.terrain_info = TerrainInfo(sigma_surface=0.2 if k % 2 else 0.1)
    m = make_model("iba", "nadir_sar_altimetry", rtsolver_options=dict(return_contributions="basic coherent"))
    one = reduced()
    both = m.run(one, sps)
    assert on_host.calls == 1     # a ragged batch with two distinct sigma_surface: one launch
    assert both.data.dims == ("snowpack", "contribution", "delay", "doppler_frequency", "theta_inc", "theta")
    assert both.data.shape == (5, 6, 8, 4, 1, 1) and both.z_gate.shape == (5, 8) and len(on_host.last_params.table_sigma) == 2
    assert list(both.contributions()) == contribution_names("basic coherent", 1)
    single = m.run(one, sps[3])
    assert np.array_equal(single.data.values, both.data.values[3]) and np.array_equal(single.z_gate.values, both.z_gate.values[3], equal_nan=True)
    ddm = both.delay_doppler_map(contribution="volume", snowpack=3)
    assert ddm.shape == (8, 4) and np.array_equal(ddm.values, 4 * np.pi * single.data.values[4, :, :, 0, 0])
    assert np.allclose(np.ravel(both.waveform(snowpack=3)), 4 * np.pi * single.data.values[5, :, :, 0, 0].sum(axis=1), rtol=1e-14, atol=0)
    assert np.allclose(both.gate, np.arange(8) + 0.375, atol=1e-12) and np.allclose(both.doppler_bin, [-1.5, -0.5, 0.5, 1.5], atol=1e-12)
    # a second sensor configuration is a second launch
    calls = on_host.calls
    config = dict(frequency=13.575e9, altitude=717_242, pulse_bandwidth=320e6, pulse_repetition_frequency=17825, velocity=7435, ngate=8,
                  ndoppler=4, nominal_gate=3, beamwidth_alongtrack=(1.08 + 1.2) / 2, beamwidth_acrosstrack=(1.08 + 1.2) / 2, doppler_window="hamming")
    two = m.run(sar_altimeter_list.make_multi_channel_altimeter({"level": config, "rolled": dict(config, roll_angle_deg=0.1)}, None), sps[:2])
    assert on_host.calls == calls + 2 and two.data.dims[:2] == ("channel", "snowpack") and two.data.shape[:3] == (2, 2, 6)
    assert np.array_equal(two.data.values[0], both.data.values[:2]) and not np.array_equal(two.data.values[1], both.data.values[:2])
    # "full": one contribution per interface; snowpacks of different depths are nested, not stacked
    full = make_model("iba", "nadir_sar_altimetry", rtsolver_options=dict(return_contributions="full"))
    same = full.run(one, [sps[0], sps[3]])
    assert list(same.contributions()) == ["interface 0", "volume", "total"] and same.data.shape[:2] == (2, 3)
    # oversampled
    fine = make_model("iba", "nadir_sar_altimetry", rtsolver_options=dict(return_oversampled=True)).run(one, sps[0])
    assert fine.data.shape == (32, 16, 1, 1)
    coarse = fine.data.values[:, :, 0, 0].reshape(8, 4, 4, 4).mean(axis=(1, 3))
    assert np.allclose(coarse, both.data.values[0, -1, :, :, 0, 0], rtol=1e-12, atol=0)
    # error handling: one element marked, its neighbours intact
    warm = snowpack(thickness=(0.5, 0.5))
    warm.layers[1].temperature = 280.0
    with pytest.raises(SMRTError, match="Invalid layer properties"):
        m.run(one, [sps[0], warm, sps[1]])
    nan = make_model("iba", "nadir_sar_altimetry", rtsolver_options=dict(return_contributions="basic coherent", error_handling="nan"))
    marked = nan.run(one, [sps[0], warm, sps[1]])
    assert np.all(np.isnan(marked.data.values[1])) and np.array_equal(marked.data.values[[0, 2]], both.data.values[[0, 1]])
    # files
    path = str(tmp_path / "ddm.nc")
    both.save(path)
    back = open_result(path)
    assert isinstance(back, AltimetryResult) and back.data.dims == both.data.dims and np.array_equal(back.data.values, both.data.values)
    assert np.array_equal(back.z_gate.values, both.z_gate.values, equal_nan=True) and np.allclose(back.gate, both.gate, rtol=1e-15)
    assert np.allclose(back.doppler_bin, both.doppler_bin, rtol=1e-15) and list(back.contributions()) == list(both.contributions())


def test_a_group_over_the_budget_is_launched_in_parts(on_host, monkeypatch):
    """The maps and the tables of a part stay inside OUTPUT_BUDGET; the parts together are the unsplit result, bitwise."""
    from smrt_amd.rtsolver import nadir_sar_altimetry as module
    from smrt_amd.rtsolver.nadir_sar_altimetry import NadirSARAltimetry

    sps = [snowpack(thickness=(0.5, 0.4 + 0.1 * k, 0.5)[:1 + k % 3]) for k in range(5)]
    for k, sp in enumerate(sps):
        sp.terrain_info = TerrainInfo(sigma_surface=0.05 * (k + 1))       # one sigma_surface per snowpack
    m = make_model("iba", "nadir_sar_altimetry", rtsolver_options=dict(return_contributions="basic coherent"))
    sensor = reduced()
    whole = m.run(sensor, sps)
    assert on_host.calls == 1 and len(on_host.last_params.table_sigma) == 5
    maps, tables = 6 * 8 * 4 * 8, 2 * 32 * 16 * 8                        # bytes of the maps and of the tables of one snowpack
    monkeypatch.setattr(module, "OUTPUT_BUDGET", 2 * (maps + tables))
    solver = NadirSARAltimetry(return_contributions="basic coherent")
    parts = solver.solve_plan(m, m.plan(sensor, sps))
    assert solver.launches == 3 and on_host.calls == 4 and len(on_host.last_params.table_sigma) == 1
    assert np.array_equal(parts.data.values, whole.data.values) and np.array_equal(parts.z_gate.values, whole.z_gate.values, equal_nan=True)
    assert np.array_equal(parts.other_data["ks"].values, whole.other_data["ks"].values, equal_nan=True)


def test_pitch_and_roll_finding_of_the_reference():
    """dinardo18.py evaluates the tanh term of D18 eq. 26 and discards it: for roll > 0 the correction is the constant
    2 gamma_y roll^2, for roll <= 0 there is none.  The restatement (and the device) reproduce what the reference computes."""
    plus, minus = reduced(roll_angle_deg=0.1), reduced(roll_angle_deg=-0.1)
    a, b = surface_map(plus, 4, 4, 0.2, 200.0), surface_map(minus, 4, 4, 0.2, 200.0)
    assert np.abs(a - b).max() > 1e-6 * np.abs(a).max()          # (a physical model would be even in the roll angle)
    assert np.array_equal(surface_map(plus, 4, 4, 0.0, 200.0), surface_map(minus, 4, 4, 0.0, 200.0))


def test_header_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "smrt_dort.h")).read()
    body = header[header.index("typedef struct smrt_sar_params {"):header.index("} smrt_sar_params;")]
    declared = [line.split(";")[0].split()[-1].lstrip("*") for line in body.splitlines()[1:] if ";" in line]
    assert declared == [name for name, _ in _native.SarParams._fields_]
    lib = _native.load_library()
    for name in ("out_stride", "run_pairs", "upload_pairs", "launch", "sync", "download", "kernel_ms", "abi"):
        assert "smrt_sar_" + name in _native.EXPORTED_SYMBOLS and hasattr(lib, "smrt_sar_" + name) and ("smrt_sar_" + name + "(") in header
    assert _native.sar_params_layout() == _native.sar_abi_layout(lib)
