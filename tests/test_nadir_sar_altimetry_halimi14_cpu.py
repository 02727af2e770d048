"""The delay-Doppler model of Halimi et al. 2014 in the nadir SAR altimetry solver, without a GPU: the NumPy restatement (direct
sums) against every fixture the reference made, the DEVICE arithmetic (smrt_amd/csrc/nadir_sar_altimetry_kernel.hpp: sar_h14_*,
sar_combine_model) compiled with g++ against every fixture and against the restatement, the table alone against the reference's
own delay_doppler_map, the options and refusals, the appended fields of the C ABI, and Dinardo18 through the same build, bit for
bit what the Dinardo18-only entry point gives.

Bars: EVERY sample of every contribution within 1e-8 x the largest value of the case's total map (the project's bar for this
solver; direct summation sits near 1e-15 of the peak from the reference's FFTs); the table 1e-8 x its own peak; z_gate and the axes
1e-12 relative.  Measured: profiles/nadir_sar_altimetry_halimi14_parity.txt."""
import ctypes as C
import os
import types
import warnings

import numpy as np
import pytest

from smrt_amd import _native, make_model
from smrt_amd.core.error import SMRTError, SMRTWarning
from smrt_amd.core.result import AltimetryResult
from smrt_amd.core.terrain import TerrainInfo
from smrt_amd.inputs import sar_altimeter_list
from smrt_amd.inputs.make_medium import make_interface, make_snowpack, make_soil
import nadir_sar_altimetry_restatement as dinardo
from host_build import host_library
from nadir_sar_altimetry_halimi14_restatement import (CASES, REL_BAR, build_snowpack, case_by_name, compensation_shifts, halimi14_table,
                                                      impulse_response, make_sensor, model_options, solve_case, solver_options)
from test_nadir_sar_altimetry_cpu import (HostContext, assert_axes, assert_close, assert_map, assert_vertical, map_of,
                                          host_lib as dinardo_host_lib)  # noqa: F401  (dinardo_host_lib is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
IDS = dict(ids=lambda c: c["name"])
API = types.SimpleNamespace(make_snowpack=make_snowpack, make_soil=make_soil, make_interface=make_interface,
                            sar_altimeter_list=sar_altimeter_list, TerrainInfo=TerrainInfo)
H14 = dict(delay_doppler_model="halimi14")


def golden(case):
    return np.load(os.path.join(GOLDEN, "nadir_sar_altimetry_halimi14_" + case["name"] + ".npz"))


_RESTATED = {}


def restated(case):
    """The restatement of a case, computed once and shared (never modified)."""
    if case["name"] not in _RESTATED:
        _RESTATED[case["name"]] = solve_case(case, API)
    return _RESTATED[case["name"]]


def assert_table(table, reference, what):
    peak = float(np.abs(reference).max())
    err = float(np.abs(table - reference).max())
    print(f"{what}: table, largest difference {err:.3e}, peak {peak:.3e}, ratio to the bar {err / peak / REL_BAR:.3e}")
    assert table.shape == reference.shape and np.all(np.isfinite(table)) and err <= REL_BAR * peak, (what, err, peak)


# ---- the device source on the CPU, both models -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_lib():
    lib = host_library("libsmrt_sar_halimi14_host.so", "nadir_sar_altimetry_halimi14_host.cpp")
    lib.smrt_sar_host_run.restype = lib.smrt_sar_host_run_table.restype = C.c_int32
    lib.smrt_sar_host_refusal.restype = C.c_char_p
    lib.layers = host_library("libsmrt_lrm_host.so", "nadir_lrm_altimetry_host.cpp")
    lib.layers.smrt_lrm_host_layers.restype = C.c_int32
    return lib


class TableContext(HostContext):
    """HostContext that also keeps the first table of the last Halimi14 run, [delays][Doppler]."""

    def sar_run(self, batch, params, pairs=None):
        self.calls += 1
        o = _native.SarOutput(batch, params, batch.n_pairs)
        s = params.struct
        self.table = np.full((s.ngate * s.oversampling_time, s.ndoppler * s.oversampling_doppler), np.nan)
        assert self.lib.smrt_sar_host_run_table(C.byref(batch.struct), C.byref(s), *o.pointers(), self.table.ctypes.data_as(C.POINTER(C.c_double))) == 0
        if pairs is not None:
            for name in ("values", "status", "z_gate", "layers", "vertical", "echo"):
                setattr(o, name, getattr(o, name)[np.asarray(pairs)])
        self.last, self.last_params, self.batch = o, params, batch
        return o


@pytest.fixture()
def on_host(host_lib, monkeypatch):
    from smrt_amd.rtsolver import nadir_sar_altimetry as module

    ctx = TableContext(host_lib)
    monkeypatch.setattr(module, "get_context", lambda device=None: ctx)
    return ctx


def run_case(case):
    m = make_model("iba", "nadir_sar_altimetry", rtsolver_options=solver_options(case))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", SMRTWarning)     # (the coherent echo: test_coherent_echo_warns_and_is_added)
        return m, m.run(make_sensor(case, API), build_snowpack(case, API))


# ---- restatement against the fixtures -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, **IDS)
def test_restatement_reproduces_the_fixture(case):
    g, sol = golden(case), restated(case)
    assert list(g["contributions"]) == sol["contributions"]
    assert_map(sol["ddm"], g["ddm"], "restatement " + case["name"])
    assert_axes(sol, g, "restatement " + case["name"])
    assert_vertical(sol["vertical"], sol["echo"], g, "restatement " + case["name"])
    assert_close(sol["t_interface"], g["t_interface"], 1e-12, "t_interface")
    if "table" in g:
        assert_table(sol["table"], g["table"], "restatement " + case["name"])
    sensor, opt = make_sensor(case, API), dict(dinardo.DEFAULTS, **solver_options(case))
    assert np.array_equal(compensation_shifts(sensor, opt["oversampling_time"], opt["oversampling_doppler"]), g["compensation"])


def test_fixtures_cover_what_they_must():
    gs = {c["name"]: golden(c) for c in CASES}
    assert [c["name"] for c in CASES] == ["n16_d16_os1", "n63_d60", "n65_d68_os4_full_oversampled", "widening2", "plrm", "shifted_out",
                                          "narrow_pdf", "last_column", "iem_surface", "cryosat2_sarm", "last_sample"]
    assert gs["n16_d16_os1"]["table"].shape == (16, 16) and gs["n63_d60"]["table"].shape == (63, 60) and gs["n63_d60"]["ddm"].shape == (4, 63, 20)
    assert gs["n65_d68_os4_full_oversampled"]["ddm"].shape == (2 * 2 + 2, 260, 68) and gs["cryosat2_sarm"]["ddm"].shape == (1, 128, 64)
    assert len(gs["widening2"]["last_column"]) == 2 * 64 and gs["widening2"]["ddm"].shape[0] == 6 and gs["widening2"]["echo"].shape[1] == 4
    out = gs["shifted_out"]
    assert out["compensation"].max() >= 64 and np.all(out["table"][:, out["compensation"] >= 64] == 0) and np.abs(out["table"]).max() > 0
    assert np.all(np.abs(gs["plrm"]["table"]).max(axis=0) > 0)
    assert gs["last_column"]["last_column"].min() < 0 and len(gs["last_column"]["last_column"]) == 16 * 12
    assert restated(case_by_name("last_sample"))["shift"][1] == 31
    assert "table" not in gs["cryosat2_sarm"] and all("table" in g for n, g in gs.items() if n != "cryosat2_sarm")
    coherent = gs["widening2"]["ddm"]
    assert coherent[1].max() > 1e-3 * coherent[-1].max()                      # the coherent surface echo counts


def test_last_column_finding_of_the_reference():
    """halimi14.py:diff_cyclic sets the last Doppler column of the difference to phi[0] - phi[1]: not the cyclic phi[0] - phi[-1]
    (which would be negative too, and about Nb times larger), and of the sign opposite to every other column."""
    case = case_by_name("last_column")
    sensor, g = make_sensor(case, API), golden(case)
    fsir = impulse_response(sensor, 1, 1, 12)
    assert np.allclose(fsir[:, -1], g["last_column"], rtol=1e-12, atol=0) and fsir[:, -1].min() < 0 and fsir[:, :-1].min() >= 0
    rows = fsir[:, -1] < 0
    assert np.allclose(fsir[rows, -1], -fsir[rows, 0], rtol=1e-12, atol=0)      # phi[0] - phi[1] = -(phi[1] - phi[0])


# ---- the device source on the CPU ---------------------------------------------------------------------------------------
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
    # the table alone: the reference's own delay_doppler_map where the fixture holds it, the restatement everywhere
    if "table" in g:
        assert_table(on_host.table, g["table"], "device source on the CPU " + case["name"])
    assert_table(on_host.table, restated(case)["table"], "device source against the restatement " + case["name"])
    p = on_host.last_params.struct
    assert (p.delay_doppler_model, bool(p.slant_range_correction), p.delay_window_widening) == (1,) + tuple(model_options(case).values())


# ---- the Python layer -------------------------------------------------------------------------------------------------------
def test_halimi14_is_selectable():
    from smrt_amd.rtsolver.delay_doppler_model.halimi14 import Halimi14
    from smrt_amd.rtsolver.nadir_sar_altimetry import Halimi14 as exported, NadirSARAltimetry

    assert exported is Halimi14
    for model in ("halimi14", "Halimi14", Halimi14):
        s = NadirSARAltimetry(delay_doppler_model=model)
        assert (s.delay_doppler_model, s.slant_range_correction, s.delay_window_widening, s.oversampling_time, s.oversampling_doppler) == \
            ("halimi14", True, 1, 4, 4)
    s = NadirSARAltimetry(delay_doppler_model_options=dict(slant_range_correction=False, delay_window_widening=3, ptr_time="sinc^2", ptr_doppler=None), **H14)
    assert (s.slant_range_correction, s.delay_window_widening) == (False, 3)
    assert NadirSARAltimetry().delay_doppler_model == "dinardo18" and NadirSARAltimetry(delay_doppler_model="dinardo18").delay_doppler_model == "dinardo18"


def test_options_and_refusals():
    from smrt_amd.rtsolver.nadir_sar_altimetry import NadirSARAltimetry

    for bad in (dict(ptr_time="gaussian"), dict(ptr_doppler="gaussian-smrt"), dict(ptr_doppler="hamming")):
        with pytest.raises(SMRTError, match="sinc"):
            NadirSARAltimetry(delay_doppler_model_options=bad, **H14)
    for bad in (0, -1, 1.5, True, "2"):
        with pytest.raises(SMRTError, match="delay_window_widening"):
            NadirSARAltimetry(delay_doppler_model_options=dict(delay_window_widening=bad), **H14)
    with pytest.raises(SMRTError, match="ptr_time, ptr_doppler, slant_range_correction and delay_window_widening"):
        NadirSARAltimetry(delay_doppler_model_options=dict(grid_space=300), **H14)
    # every other model keeps being refused, and the message names both
    Ray15 = type("Ray15", (), {})
    for bad in ("ray15", Ray15, "wingham04", "wingham18", "boy17", "buchhaupt18", "landy19", 3):
        with pytest.raises(SMRTError, match="Dinardo18.*Halimi14"):
            NadirSARAltimetry(delay_doppler_model=bad)
    # Dinardo18 keeps its own options
    for bad in (dict(ptr_time="sinc^2"), dict(slant_range_correction=False), dict(delay_window_widening=2)):
        with pytest.raises(SMRTError, match="Dinardo18"):
            NadirSARAltimetry(delay_doppler_model_options=bad)


def reduced(**kwargs):
    return make_sensor(dict(sensor=dict(ngate=8, nominal_gate=3, ndoppler=16, **kwargs)), API)


_GO = dict(roughness_rms=0.005, corr_length=0.10)


def snowpack(thickness=(1.0,), interface=None, substrate=None, terrain_info="default"):
    n = len(thickness)
    itf = [make_interface("geometrical_optics_backscatter", **_GO) for _ in range(n)] if interface is None else interface
    sp = make_snowpack(list(thickness), "exponential", density=[300.0, 350.0, 400.0][:n], temperature=[258.0, 260.0, 262.0][:n],
                       corr_length=2e-4, interface=itf, substrate=substrate)
    sp.terrain_info = TerrainInfo(sigma_surface=0.2) if terrain_info == "default" else terrain_info
    return sp


def quiet(model, *args):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", SMRTWarning)
        return model.run(*args)


def test_snowpack_checks_follow_the_tabulated_branch(on_host):
    m = make_model("iba", "nadir_sar_altimetry", rtsolver_options=H14)
    sensor = reduced()
    iem = [make_interface("iem_fung92", roughness_rms=5e-4, corr_length=1e-2)]
    assert np.all(np.isfinite(quiet(m, sensor, snowpack(interface=iem)).data.values))          # no mean_square_slope is required ...
    with pytest.raises(SMRTError, match="mean_square_slope"):                                     # ... which Dinardo18 refuses
        make_model("iba", "nadir_sar_altimetry").run(sensor, snowpack(interface=iem))
    for interface in ([None], [make_interface("transparent")]):
        with pytest.raises(SMRTError, match="roughness_rms"):
            m.run(sensor, snowpack(interface=interface))
    with pytest.raises(SMRTError, match="roughness_rms"):
        m.run(sensor, snowpack(substrate=make_soil("flat", complex(5.0, 0.5), temperature=270.0)))
    with pytest.raises(SMRTError, match="Halimi14.*normally-distributed"):
        m.run(sensor, snowpack(terrain_info=TerrainInfo(distribution="lognormal", sigma_surface=0.2)))
    with pytest.raises(SMRTError, match="dem"):
        m.run(sensor, snowpack(terrain_info=TerrainInfo(dem=np.zeros((2, 2)))))
    with pytest.raises(SMRTError, match="slope_angle"):
        m.run(sensor, snowpack(terrain_info=TerrainInfo(slope_angle=0.01)))
    odd = reduced()
    odd.ndoppler = 17
    with pytest.raises(SMRTError, match="even"):
        m.run(odd, snowpack())
    late = snowpack(thickness=(3.4, 1.0))
    with pytest.raises(SMRTError, match="later than the window"):
        quiet(m, sensor, late)


def test_coherent_echo_warns_and_is_added(on_host, capsys):
    m = make_model("iba", "nadir_sar_altimetry", rtsolver_options=dict(return_contributions="basic coherent", **H14))
    with pytest.warns(SMRTWarning, match="not compatible with coherent backscatter"):
        res = m.run(reduced(), snowpack())
    assert capsys.readouterr().out == ""                                                        # warned, not printed
    w = res.data.values[..., 0, 0]
    surface = w[0] / on_host.last.echo[0, 0, 2]
    assert w[1].max() > 0 and np.allclose(w[1], surface * on_host.last.echo[0, 0, 1], rtol=1e-13, atol=0)   # the same shifted map


def test_a_unit_surface_echo_at_shift_zero_is_the_table(on_host):
    """'full' contributions: the row of the surface is the table times its incoherent echo, sample by sample."""
    m = make_model("iba", "nadir_sar_altimetry", rtsolver_options=dict(return_contributions="full", return_oversampled=True, **H14))
    res = quiet(m, reduced(), snowpack())
    assert np.array_equal(res.data.values[0, :, :, 0, 0], on_host.table * on_host.last.echo[0, 0, 2])
    sensor = reduced()
    assert_table(on_host.table, halimi14_table(sensor, 4, 4, 0.2), "reduced sensor")


def test_batches_groups_and_error_handling(on_host):
    sps = [snowpack(thickness=(0.5, 0.4 + 0.1 * k, 0.5)[:1 + k % 3]) for k in range(5)]
    for k, sp in enumerate(sps):
        sp.terrain_info = TerrainInfo(sigma_surface=0.2 if k % 2 else 0.1)
    options = dict(return_contributions="basic coherent", delay_doppler_model_options=dict(delay_window_widening=2), **H14)
    m, one = make_model("iba", "nadir_sar_altimetry", rtsolver_options=options), reduced()
    both = quiet(m, one, sps)
    assert on_host.calls == 1 and len(on_host.last_params.table_sigma) == 2      # a ragged batch, two sigma_surface: one launch
    assert both.data.shape == (5, 6, 8, 16, 1, 1) and both.z_gate.shape == (5, 8)
    single = quiet(m, one, sps[3])
    assert np.array_equal(single.data.values, both.data.values[3]) and np.array_equal(single.z_gate.values, both.z_gate.values[3], equal_nan=True)
    fine = quiet(make_model("iba", "nadir_sar_altimetry", rtsolver_options=dict(options, return_oversampled=True)), one, sps[0])
    coarse = fine.data.values[:, :, :, 0, 0].reshape(6, 8, 4, 16, 4).mean(axis=(2, 4))
    assert fine.data.shape == (6, 32, 64, 1, 1) and np.allclose(coarse, both.data.values[0, :, :, :, 0, 0], rtol=1e-12, atol=0)
    # the other model on the same snowpacks is another group: another launch, another answer
    calls = on_host.calls
    other = make_model("iba", "nadir_sar_altimetry", rtsolver_options=dict(return_contributions="basic coherent")).run(one, sps)
    assert on_host.calls == calls + 1 and other.data.shape == both.data.shape and not np.array_equal(other.data.values, both.data.values)
    # error handling: one element marked, its neighbours intact
    warm = snowpack(thickness=(0.5, 0.5))
    warm.layers[1].temperature = 280.0
    with pytest.raises(SMRTError, match="Invalid layer properties"):
        quiet(m, one, [sps[0], warm, sps[1]])
    marked = quiet(make_model("iba", "nadir_sar_altimetry", rtsolver_options=dict(options, error_handling="nan")), one, [sps[0], warm, sps[1]])
    assert np.all(np.isnan(marked.data.values[1])) and np.array_equal(marked.data.values[[0, 2]], both.data.values[[0, 1]])


def test_the_budget_counts_one_table_per_sigma_surface(on_host, monkeypatch):
    from smrt_amd.rtsolver import nadir_sar_altimetry as module
    from smrt_amd.rtsolver.nadir_sar_altimetry import NadirSARAltimetry

    sps = [snowpack(thickness=(0.5, 0.4 + 0.1 * k, 0.5)[:1 + k % 3]) for k in range(5)]
    for k, sp in enumerate(sps):
        sp.terrain_info = TerrainInfo(sigma_surface=0.05 * (k + 1))
    m, sensor = make_model("iba", "nadir_sar_altimetry", rtsolver_options=H14), reduced()
    whole = quiet(m, sensor, sps)
    maps, table = 8 * 16 * 8, 32 * 64 * 8           # bytes of the map and of the ONE table of a snowpack; the widened response once
    monkeypatch.setattr(module, "OUTPUT_BUDGET", table + 2 * (maps + table))
    solver = NadirSARAltimetry(**H14)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", SMRTWarning)
        parts = solver.solve_plan(m, m.plan(sensor, sps))
    assert solver.launches == 3 and len(on_host.last_params.table_sigma) == 1     # (Dinardo18's pair of tables would need five)
    assert np.array_equal(parts.data.values, whole.data.values)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals(host_lib, on_host):
    quiet(make_model("iba", "nadir_sar_altimetry", rtsolver_options=H14), reduced(), snowpack())
    params = on_host.last_params

    def refusal(**changes):
        p = _native.SarParams.from_buffer_copy(params.struct)
        for k, v in changes.items():
            setattr(p, k, v)
        return host_lib.smrt_sar_host_refusal(C.byref(on_host.batch.struct), C.byref(p))

    assert refusal() is None and refusal(delay_doppler_model=0) is None
    assert b"unknown delay_doppler_model" in refusal(delay_doppler_model=2) and b"unknown delay_doppler_model" in refusal(delay_doppler_model=-1)
    assert b"delay_window_widening" in refusal(delay_window_widening=0)
    assert refusal(delay_doppler_model=0, delay_window_widening=0) is None        # Dinardo18 reads none of the appended fields
    assert b"invalid sensor" in refusal(burst_duration=0.0) and b"local data share" in refusal(delay_window_widening=4096)
    assert b"even" in refusal(ndoppler=17)


def test_header_and_binding_agree_on_the_appended_fields():
    header = open(os.path.join(ROOT, "include", "smrt_dort.h")).read()
    body = header[header.index("typedef struct smrt_sar_params {"):header.index("} smrt_sar_params;")]
    declared = [line.split(";")[0].split()[-1].lstrip("*") for line in body.splitlines()[1:] if ";" in line]
    names = [name for name, _ in _native.SarParams._fields_]
    assert declared == names
    appended = ["delay_doppler_model", "slant_range_correction", "delay_window_widening", "reserved2", "h14_pu", "h14_gamma", "burst_duration"]
    assert names[names.index("row_map") + 1:] == appended and names.index("reserved") == names.index("table_sigma") - 1
    zero = _native.SarParams()
    assert zero.delay_doppler_model == 0 == _native.SAR_MODELS["dinardo18"] and _native.SAR_MODELS["halimi14"] == 1
    assert "SMRT_SAR_DINARDO18 = 0, SMRT_SAR_HALIMI14 = 1" in header
    lib = _native.load_library()
    assert _native.sar_params_layout() == _native.sar_abi_layout(lib) and len(_native.sar_params_layout()) == len(names) + 1
    # a caller of the layout before this model: its fields have not moved
    assert [getattr(_native.SarParams, n).offset for n in ("altitude", "ngate", "reserved", "table_sigma", "row_map")] == [0, 136, 164, 168, 192]


# ---- Dinardo18 through the build that carries both models --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pitch_roll_full_coherent", "n63_d60_basic"])
def test_dinardo18_is_bit_for_bit_what_it_was(name, host_lib, dinardo_host_lib, monkeypatch):  # noqa: F811
    """The map kernel is a template over the model now; its Dinardo18 instantiation is the arithmetic of before.  The entry point
    of tests/hostemu/nadir_sar_altimetry_host.cpp reaches it through sar_combine_item as it always did, the new one through
    sar_combine_model<kSarDinardo18> next to the Halimi14 code: both against each other bit for bit, and against the fixture."""
    from smrt_amd.rtsolver import nadir_sar_altimetry as module

    case = dinardo.case_by_name(name)
    maps = []
    for lib in (dinardo_host_lib, host_lib):
        ctx = HostContext(lib)
        monkeypatch.setattr(module, "get_context", lambda device=None, ctx=ctx: ctx)
        m = make_model("iba", "nadir_sar_altimetry", rtsolver_options=dinardo.solver_options(case))
        res = m.run(dinardo.make_sensor(case, API), dinardo.build_snowpack(case, API))
        maps.append((map_of(res).copy(), ctx.last.z_gate.copy(), ctx.last.echo.copy()))
    for a, b in zip(*maps):
        assert np.array_equal(a, b, equal_nan=True)
    g = np.load(os.path.join(GOLDEN, "nadir_sar_altimetry_" + name + ".npz"))
    assert_map(maps[1][0], g["ddm"], "Dinardo18 through the build of both models " + name)
