"""The iterative first-order solver without a GPU: plugin resolution and options, the refusals, the packing of the extras,
the ctypes struct against the library's self-description, the NumPy restatement against every fixture, and the DEVICE
arithmetic (smrt_amd/csrc/first_order_kernel.hpp) compiled with g++ against every fixture.

Tolerance: every element within SIGMA_RTOL = 1e-8 of the solve's largest co-polarised total (the project's bar for sigma0
against the reference); the contributions and backscatter_layer on that same scale.  Layer scalars: eps 1e-12, ks 1e-11,
ka 1e-10 relative (tests/test_gpu_parity.py)."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import smrt_amd
from first_order_restatement import CASES, CONTRIBUTIONS, SIGMA_RTOL, build_snowpack, solve_case
from host_build import host_library
from smrt_amd import make_model, sensor_list
from smrt_amd import _native
from smrt_amd.core.error import SMRTError
from smrt_amd.inputs.make_medium import make_interface, make_snowpack, make_soil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def api():
    from smrt_amd.substrate.reflector import make_reflector
    from smrt_amd.substrate.transparent import Transparent

    return types.SimpleNamespace(make_snowpack=make_snowpack, make_interface=make_interface, make_soil=make_soil,
                                 make_reflector=make_reflector, transparent_substrate=Transparent)


def golden(case):
    return np.load(os.path.join(GOLDEN, "first_order_" + case["name"] + ".npz"))


def scale_of(g):
    total = g["contributions"][0]
    return max(total[:, 0, 0].max(), total[:, 1, 1].max())


def assert_matches_fixture(case, contributions4, layer_backscatter, layers=None, what=""):
    """contributions4 [4, n, 2, 2], layer_backscatter [L + 1, n, 2, 2], layers [L, >= 4] = Re eps, Im eps, ks, ka.  Returns
    the worst error relative to the scale."""
    g = golden(case)
    scale = scale_of(g)
    ref = g["contributions"]
    err = max(np.abs(contributions4 - ref[1:]).max(), np.abs(contributions4.sum(axis=0) - ref[0]).max()) / scale
    theta = np.deg2rad(case["theta"])
    # backscatter_layer is a sigma0 (4 pi mu x intensity): measured against the total on that same footing
    err_layer = np.abs(layer_backscatter - g["backscatter_layer"]).max() / (4 * np.pi * np.cos(theta).min() * scale)
    print(f"{what} {case['name']}: contributions {err:.2e}, backscatter_layer {err_layer:.2e} (of the largest co-polarised total)")
    assert err <= SIGMA_RTOL and err_layer <= SIGMA_RTOL, (case["name"], err, err_layer)
    if layers is not None:
        eps = layers[:, 0] + 1j * layers[:, 1]
        assert np.abs(eps - g["eps"]).max() <= 1e-12 * np.abs(g["eps"]).max()
        assert np.all(np.abs(layers[:, 2] - g["ks"]) <= 1e-11 * np.maximum(np.abs(g["ks"]), 1e-300) + 0.0)
        assert np.all(np.abs(layers[:, 3] - g["ka"]) <= 1e-10 * np.abs(g["ka"]))
    return max(err, err_layer)


# ---- plugin, options, refusals -----------------------------------------------------------------------------------------
def test_plugin_resolution_and_options():
    from smrt_amd.core.model import make_rtsolver
    from smrt_amd.core.plugin import import_class
    from smrt_amd.rtsolver.iterative_first_order import IterativeFirstOrder

    assert import_class("rtsolver", "iterative_first_order") is IterativeFirstOrder
    m = make_model("iba", "iterative_first_order", rtsolver_options={"return_contributions": True, "error_handling": "nan"})
    solver = m.make_rtsolver_instance()
    assert isinstance(solver, IterativeFirstOrder) and solver.return_contributions and solver.error_handling == "nan"
    assert issubclass(make_rtsolver("iterative_first_order", return_contributions=True), IterativeFirstOrder)
    assert IterativeFirstOrder._broadcast_capability == {"theta_inc", "polarization_inc", "theta", "polarization"}
    assert not IterativeFirstOrder().return_contributions and IterativeFirstOrder().error_handling == "exception"
    with pytest.raises(SMRTError):
        IterativeFirstOrder(error_handling="ignore")
    # the frequency is the only sensor axis the model has to flatten
    assert [a for a, _ in m.split_axes(sensor_list.active([13e9, 17e9], [20, 30]))] == ["frequency"]


def test_refuses_passive_sensors_and_atmospheres():
    from smrt_amd.atmosphere.simple_isotropic_atmosphere import SimpleIsotropicAtmosphere
    from smrt_amd.rtsolver.iterative_first_order import IterativeFirstOrder

    sp = make_snowpack([1.0], "exponential", density=[300.0], temperature=[260.0], corr_length=[2e-4])
    m = make_model("iba", "iterative_first_order")
    with pytest.raises(SMRTError, match="active"):
        m.run(sensor_list.passive(37e9, 55), sp)
    with pytest.raises(SMRTError, match="active"):
        IterativeFirstOrder().solve(sp, [None], sensor_list.passive(37e9, 55))
    atmosphere = SimpleIsotropicAtmosphere(tb_down=20.0, tb_up=18.0, transmittance=0.9)
    with pytest.raises(SMRTError, match="atmosphere"):
        IterativeFirstOrder().solve(sp, [None], sensor_list.active(13e9, 30), atmosphere=atmosphere)
    with pytest.raises(SMRTError, match="atmosphere"):
        m.run(sensor_list.active(13e9, 30), atmosphere + sp)


# ---- ABI and packing ---------------------------------------------------------------------------------------------------
def test_extras_struct_matches_the_library():
    lib = _native.load_library()
    mine, theirs = _native.first_order_extras_layout(), _native.first_order_abi_layout(lib)
    assert mine == theirs and mine[0] == C.sizeof(_native.FirstOrderExtras) and len(mine) == 1 + len(_native.FirstOrderExtras._fields_)
    header = open(os.path.join(ROOT, "include", "smrt_dort.h")).read()
    body = header[header.index("typedef struct smrt_first_order_extras {"):header.index("} smrt_first_order_extras;")]
    declared = [line.split(";")[0].split()[-1].lstrip("*") for line in body.splitlines()[1:] if ";" in line]
    assert declared == [name for name, _ in _native.FirstOrderExtras._fields_]
    for name in ("smrt_first_order_run_pairs", "smrt_first_order_upload_pairs", "smrt_first_order_launch", "smrt_first_order_sync",
                 "smrt_first_order_download", "smrt_first_order_kernel_ms", "smrt_first_order_abi", "smrt_first_order_out_stride"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_packing_of_the_extras():
    FS, L, T = 6, 3, 2
    slot = -np.ones((FS, L + 1), int)
    slot[1, 0], slot[1, 3], slot[4, 2] = 0, 1, 0
    values = np.arange(FS * 2 * T * 10, dtype=float).reshape(FS, 2, T, 10)
    phases = np.arange(FS * L * T * 16, dtype=float).reshape(FS, L, T, 4, 2, 2)
    x = _native.PackedFirstOrderExtras(FS, L, T, interfaces=(slot, values), phase_samples=phases)
    assert x.struct.n_interface_slots == 2 and x.slot.dtype == np.int32 and x.slot.flags.c_contiguous
    assert x.struct.host_interface_slot[1 * (L + 1) + 3] == 1 and x.struct.host_interface_slot[0] == -1
    assert x.struct.host_interface_values[((4 * 2 + 0) * T + 1) * 10 + 7] == values[4, 0, 1, 7]
    assert x.struct.host_phase_samples[((2 * L + 1) * T + 1) * 16 + 5] == phases[2, 1, 1, 1, 0, 1]
    empty = _native.PackedFirstOrderExtras(FS, L, T)
    assert not empty.struct.host_interface_slot and not empty.struct.host_phase_samples and empty.struct.n_interface_slots == 0
    with pytest.raises(SMRTError):
        _native.PackedFirstOrderExtras(FS, L, T, interfaces=(slot[:, :L], values))
    with pytest.raises(SMRTError):
        _native.PackedFirstOrderExtras(FS, L, T, interfaces=(np.where(slot == 1, 5, slot), values))
    with pytest.raises(SMRTError):
        _native.PackedFirstOrderExtras(FS, L, T, phase_samples=phases[:, :, :1])


def test_boundary_values_of_interface_objects():
    from smrt_amd.rtsolver.iterative_first_order import IterativeFirstOrder as S

    mu = np.array([0.9, 0.7])
    v = S.boundary_values(make_interface("transparent"), 13e9, 1.0, 1.5 + 0.01j, mu, mu)
    assert np.array_equal(v[:, :2], np.zeros((2, 2))) and np.array_equal(v[:, 2:6], np.ones((2, 4))) and not v[:, 6:].any()
    iem = make_interface("iem_fung92", roughness_rms=0.002, corr_length=0.05)
    v = S.boundary_values(iem, 13e9, 1.0, 1.5 + 0.01j, mu, S.snell_from_air(1.5 + 0.01j, mu))
    gamma = iem.backscatter(13e9, 1.0, 1.5 + 0.01j, mu)
    assert np.array_equal(v[:, 6], gamma[0]) and np.array_equal(v[:, 9], gamma[1]) and not v[:, 7:9].any()
    assert np.all((v[:, :6] > 0) & (v[:, :6] < 1))
    soil = make_soil("geometrical_optics_backscatter", 8 + 1j, 268.0, mean_square_slope=0.05)
    v = S.boundary_values(soil, 13e9, 1.5 + 0.01j, None, mu, None, substrate=True)
    assert not v[:, 2:6].any() and np.all(v[:, 6] > 0) and np.array_equal(v[:, 6], v[:, 9])


# ---- the restatement against the reference's fixtures --------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_matches_the_reference(case):
    sp = build_snowpack(case, api())
    (contributions, per_layer), layers = solve_case(case, sp)
    scalars = np.array([[complex(lay.eps_eff).real, complex(lay.eps_eff).imag, lay.ks, lay.ka] for lay in layers])
    assert_matches_fixture(case, contributions, per_layer, scalars, "restatement")


def test_fixtures_exercise_every_mechanism():
    """Each of the four contributions exceeds 1 % of the total co-polarised backscatter in at least one fixture; with Flat
    interfaces off nadir the order-0 term is exactly zero."""
    share = np.zeros(4)
    for case in CASES:
        g = golden(case)
        share = np.maximum(share, [max(g["contributions"][1 + c][:, 0, 0].max(), g["contributions"][1 + c][:, 1, 1].max()) / scale_of(g)
                                   for c in range(4)])
        if not case.get("interfaces") and case.get("substrate", {}).get("substrate_model", "flat") == "flat" \
                and "transparent" not in case.get("substrate", {}):
            assert np.all(g["contributions"][1] == 0.0)
    assert np.all(share > 0.01), dict(zip(CONTRIBUTIONS[1:], share))


# ---- the device arithmetic on the CPU ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_run():
    lib = host_library("libsmrt_first_order_host.so", "first_order_host.cpp")
    P = C.POINTER
    lib.smrt_first_order_host_run.argtypes = [P(_native.SmrtBatch), P(_native.FirstOrderExtras), P(C.c_int64), C.c_int64, P(C.c_double),
                                              P(C.c_int32), P(C.c_double), P(C.c_double), P(C.c_double)]
    lib.smrt_first_order_host_run.restype = C.c_int32

    def run(batch, extras=None, pairs=None):
        o = _native.FirstOrderOutput(batch, batch.n_pairs if pairs is None else len(pairs))
        if pairs is not None:
            pairs = np.ascontiguousarray(pairs, np.int64)
        rc = lib.smrt_first_order_host_run(C.byref(batch.struct), C.byref(extras.struct) if extras is not None else None,
                                           pairs.ctypes.data_as(P(C.c_int64)) if pairs is not None else None,
                                           len(pairs) if pairs is not None else -1, *o.pointers())
        assert rc == 0
        return o
    return run


def pack_case(case, run, emmodel=None):
    """(batch, extras) of a case through the solver's own packing, the host-evaluated numbers included; `run` plays the device."""
    from smrt_amd.core.model import SimulationPlan
    from smrt_amd.rtsolver.iterative_first_order import IterativeFirstOrder

    sp = build_snowpack(case, api())
    model = make_model(emmodel or case["emmodel"], "iterative_first_order")
    sensor = sensor_list.active(case["frequency"], case["theta"])
    solver = IterativeFirstOrder()
    packer = solver._packer()
    names = solver.emmodel_names(model, SimulationPlan([sensor], [sp], np.zeros(1, int), np.zeros(1, int)))
    batch = packer._pack(sensor, [sp], np.array([float(case["frequency"])]), names, {})
    return batch, solver._extras(lambda b: run(b).layers, batch, packer, sensor, [sp], [float(case["frequency"])])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_arithmetic_on_the_cpu_matches_the_reference(case, host_run):
    batch, extras = pack_case(case, host_run)
    out = host_run(batch, extras)
    assert out.status[0] == 0
    L = len(case["thickness"])
    assert_matches_fixture(case, out.values[0], out.layer_backscatter[0][:L + 1], out.layers[0][:L], "host build")
    g = golden(case)
    ke = g["ks"] + g["ka"]
    assert np.isclose(out.diag[0, 0], (g["ks"] / ke).max(), rtol=1e-9) and np.isclose(out.diag[0, 1], (ke * np.array(case["thickness"])).sum(), rtol=1e-9)


def test_device_arithmetic_with_a_host_evaluated_emmodel(host_run):
    """An emmodel outside the IBA and Rayleigh families goes the SMRT_EM_HOST route: scalars and the four phase samples per
    (layer, angle) from the object's own ks / ka / effective_permittivity / phase.  Here the object forwards to IBA, so the
    reference's IBA fixture is the expected result."""
    from oracle import dort_oracle as O

    class Forwarding:   # not IBA, not Rayleigh: nothing the device could know (the numbers are the CPU oracle's IBA)
        def __init__(self, sensor, layer):
            self._em = O.IBALayer(float(sensor.frequency), layer.frac_volume, layer.temperature, "exponential",
                                  corr_length=layer.microstructure.corr_length)

        def effective_permittivity(self):
            return self._em.eps_eff

        def ks(self, mu, npol=2):
            return self._em.ks

        def ka(self, mu, npol=2):
            return self._em.ka

        def phase(self, mu_s, mu_i, dphi, npol=2):
            return self._em.phase(mu_s, mu_i, dphi, npol)

    case = next(c for c in CASES if c["name"] == "iba_exp_L3_flat")
    batch, extras = pack_case(case, host_run, emmodel=Forwarding)
    assert extras is not None and bool(extras.struct.host_phase_samples) and (batch.layer_kind & 15 == _native.EM_CODES["host"]).all()
    out = host_run(batch, extras)
    assert out.status[0] == 0
    assert_matches_fixture(case, out.values[0], out.layer_backscatter[0][:4], None, "host emmodel")


def test_invalid_layer_gives_status_and_nan_for_that_pair_only(host_run):
    good = CASES[1]
    batch, _ = pack_case(good, host_run)
    bad = _native.PackedBatch([3, 3], np.tile(batch.thickness, (2, 1)), np.tile(batch.frac_volume, (2, 1)),
                              np.array([batch.temperature[0], [280.0, 260.0, 260.0]]), np.tile(batch.micro_p1, (2, 1)), None,
                              batch.frequency, batch.theta, mode="A", substrate=("flat", 8.0, 1.0, [268.0, 268.0]))
    out = host_run(bad)
    assert list(out.status) == [0, 5] and np.isnan(out.values[1]).all() and np.isnan(out.layer_backscatter[1]).all()
    assert_matches_fixture(good, out.values[0], out.layer_backscatter[0], out.layers[0], "next to an invalid pair")
    sparse = host_run(bad, pairs=[1, 0, 0])
    assert list(sparse.status) == [5, 0, 0] and np.array_equal(sparse.values[1], out.values[0]) and np.array_equal(sparse.values[2], out.values[0])


def test_warnings_are_collected_once_per_run():
    """_Solution.warn: one warning per kind over all device groups of a run, with the count and the worst value; snowpacks
    on a substrate never count as optically shallow."""
    import warnings

    from smrt_amd.core.error import SMRTWarning
    from smrt_amd.rtsolver.iterative_first_order import IterativeFirstOrder, _Solution

    def group(diag):
        return types.SimpleNamespace(diag=np.array(diag, float))

    sol = _Solution(IterativeFirstOrder(), [], [], np.zeros(0, int), np.zeros(0, int))
    sol.add_group(np.zeros(0, int), group([[0.2, 1.0], [0.7, 9.0], [0.6, 2.5]]), None, no_substrate=True)
    sol.add_group(np.zeros(0, int), group([[0.9, 0.1], [0.1, 0.2]]), None, no_substrate=False)
    with pytest.warns(SMRTWarning) as record:
        sol.warn()
    messages = [str(w.message) for w in record]
    assert len(messages) == 2
    assert "in 3 simulation(s)" in messages[0] and "0.90" in messages[0]
    assert "2 snowpack(s)" in messages[1] and "tau=1" in messages[1]
    quiet = _Solution(IterativeFirstOrder(), [], [], np.zeros(0, int), np.zeros(0, int))
    quiet.add_group(np.zeros(0, int), group([[0.3, 7.0]]), None, no_substrate=True)
    quiet.add_group(np.zeros(0, int), group([[0.4, 0.5]]), None, no_substrate=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error", SMRTWarning)
        quiet.warn()


def test_geometrical_optics_backscatter_keeps_the_bistatic_matrix_off_backscatter():
    """The backscatter geometry returns the closed form the first-order solver needs; every other geometry is the inherited
    full geometrical-optics matrix, so the inherited hemispherical_reflectivity still works."""
    from smrt_amd.interface.geometrical_optics import GeometricalOptics
    from smrt_amd.interface.geometrical_optics_backscatter import GeometricalOpticsBackscatter

    gob, go = GeometricalOpticsBackscatter(mean_square_slope=0.05), GeometricalOptics(mean_square_slope=0.05)
    mu = np.array([0.9, 0.7])
    back = gob.diffuse_reflection_matrix(13e9, 1.0, 3.0 + 0.1j, mu, mu, np.pi, 2)
    assert back.shape == (2, 2) and np.array_equal(back[0], gob.backscatter(1.0, 3.0 + 0.1j, mu)) and np.array_equal(back[0], back[1])
    for args in ((mu, mu, np.array([0.0, np.pi])), (np.array([0.8]), mu, np.pi), (mu, mu, 0.3)):
        a = np.asarray(gob.diffuse_reflection_matrix(13e9, 1.0, 3.0 + 0.1j, *args, 2))
        assert np.array_equal(a, np.asarray(go.diffuse_reflection_matrix(13e9, 1.0, 3.0 + 0.1j, *args, 2)))
    assert np.array_equal(gob.hemispherical_reflectivity(13e9, 1.0, 3.0 + 0.1j, mu), go.hemispherical_reflectivity(13e9, 1.0, 3.0 + 0.1j, mu))


def test_runner_passes_the_device_list_but_no_block_size():
    from smrt_amd.rtsolver.iterative_first_order import IterativeFirstOrder
    from smrt_amd.runner.hip_batch_runner import HipBatchRunner

    solver = HipBatchRunner(devices=[0], block_threads=64)._rtsolver(make_model("iba", "iterative_first_order",
                                                                                rtsolver_options={"return_contributions": True}))
    assert isinstance(solver, IterativeFirstOrder) and solver.devices == [0] and solver.return_contributions
    with pytest.raises(TypeError):
        IterativeFirstOrder(block_threads=64)
