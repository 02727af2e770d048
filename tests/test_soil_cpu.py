"""Soil substrates (Wegmuller, QNH, Choudhury) and soil / bedrock permittivities without a GPU: the host classes against what
the reference returned (tests/golden/make_soil_fixtures.py), the packing, and the DEVICE source under the CPU emulators of
tests/hostemu against the reference's brightness temperatures.

Tolerances: permittivities 1e-12 relative and the substrate protocol 1e-13 (the same formula in the same precision);
brightness temperatures 1e-6 K, the package's contract, for DORT on every pipeline variant and for every order of
successive_order (profiles/successive_order_parity.txt)."""
import ctypes as C
import warnings

import numpy as np
import pytest

from conftest import EmulatedContext, load_golden
from soil_cases import (BEDROCK_FREQUENCIES, EDGE, EDGE_SO_OPTIONS, PERMITTIVITY_POINTS, SOIL_MODELS, WEGMULLER_CASES, WEGMULLER_SNOW)
from test_reference_binding import smrt_ref  # noqa: F401  (the reference package where it is present, else a skip)
from test_solver_refusals_cpu import FO, FO_SUBSTRATE, MF, SO, SOA, refusal  # noqa: F401  (the CPU build of the refusals)
from test_successive_order_cpu import host_lib, host_run  # noqa: F401  (the CPU build of the successive-order kernels)

from smrt_amd import make_model, make_snowpack, make_soil, sensor_list
from smrt_amd.core.error import SMRTError

TB_ATOL = 1e-6


# ---- builders ---------------------------------------------------------------------------------------------------------------
def edge_substrate(k):
    from smrt_amd.inputs.make_medium import make_soil_substrate

    spec = EDGE["substrates"][k]
    return make_soil_substrate(spec["model"], spec["permittivity_model"], spec["temperature"], **spec["soil"], **spec["parameters"])


def edge_snowpack(k, substrate="own"):
    snow = EDGE["snow"][k]
    return make_snowpack(snow["thickness"], "exponential", density=snow["density"], temperature=snow["temperature"],
                         corr_length=snow["corr_length"], substrate=edge_substrate(k) if substrate == "own" else substrate)


def wegmuller_snowpack(model):
    soil = dict(WEGMULLER_SNOW["soil"]) if model != "soil_permittivity_montpetit08" else {}
    substrate = make_soil("soil_wegmuller", model, WEGMULLER_SNOW["soil_temperature"], roughness_rms=WEGMULLER_SNOW["roughness_rms"], **soil)
    return make_snowpack(WEGMULLER_SNOW["thickness"], "sticky_hard_spheres", density=WEGMULLER_SNOW["density"],
                         temperature=WEGMULLER_SNOW["temperature"], radius=WEGMULLER_SNOW["radius"],
                         stickiness=WEGMULLER_SNOW["stickiness"], substrate=substrate)


def pack_edge(n_max_stream, solver_class=None, emitting=True, **options):
    """The F = 2, S = 3 batch of soil_edge, one snowpack per substrate kind: three one-kind batches in input order."""
    from smrt_amd.rtsolver.dort import DORT

    solver = (solver_class or DORT)(n_max_stream=n_max_stream, **options)
    packer = solver if solver_class is None else solver._packer()
    sensor = sensor_list.passive(EDGE["frequency"][0], EDGE["theta"])
    batches = [packer._pack(sensor, [edge_snowpack(k)], np.array(EDGE["frequency"]), "iba") for k in range(3)]
    for batch in batches:
        if not emitting:
            batch.sub_T[:] = 0.0   # substrate_temperature <= 0: the substrate reflects and does not emit (include/smrt_dort.h)
    return batches, solver


@pytest.fixture(scope="module")
def emu():
    ctx = EmulatedContext()
    ctx.lib.smrt_emu_run.restype = C.c_int
    return ctx.lib


def emu_run(lib, batch, pipeline, nt, order=0):
    n = batch.n_pairs
    out, st = np.empty((n,) + batch.out_shape()), np.empty(n, np.int32)
    C.c_int.in_dll(lib, "smrt_emu_pipeline").value = pipeline
    try:
        rc = lib.smrt_emu_run(C.byref(batch.struct), 0, n, nt, order, out.ctypes.data_as(C.POINTER(C.c_double)),
                              st.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None)
    finally:
        C.c_int.in_dll(lib, "smrt_emu_pipeline").value = 1
    assert rc == 0
    return out, st


# every pipeline variant the passive emulator tests run: fused, two- and four-slot split, register-resident finish, the eight-
# and the four-wavefront strip finish, in three fiber orders.  (The emulator's entry points of the strip and register-resident
# kernels are their SOIL instances, the ones the library launches for a soil batch: csrc/dort_layout.hpp.)
PIPELINES = [(0, 64, 0), (1, 128, 1), (2, 256, 2), (3, 256, 0), (5, 256, 1), (6, 256, 2)]


# ---- permittivities ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SOIL_MODELS))
def test_soil_permittivities_against_the_reference_table(name):
    from smrt_amd.permittivity import soil

    table = load_golden("soil_permittivity_table")[name]
    points = PERMITTIVITY_POINTS[name]
    function = getattr(soil, name)
    assert function.required_arguments == list(SOIL_MODELS[name])
    one_by_one = np.array([complex(function(p["frequency"], **{a: p[a] for a in SOIL_MODELS[name]})) for p in points])
    assert np.abs(one_by_one - table).max() <= 1e-12 * np.abs(table).max() and np.all(np.abs(one_by_one / table - 1) < 1e-12)
    # vectorised over the snowpacks of a batch: the columns of all points at one frequency, one complex value per element
    columns = {a: np.array([p[a] for p in points]) for a in SOIL_MODELS[name]}
    for p, expected in zip(points, one_by_one):
        together = function(p["frequency"], **columns)
        assert together.shape == (len(points),) and np.iscomplexobj(together)
        assert abs(together[points.index(p)] - expected) <= 1e-15 * abs(expected)


def test_bedrock_permittivities_against_the_reference_table():
    from smrt_amd.permittivity import bedrock

    table = load_golden("soil_permittivity_table")
    names = [str(n) for n in table["bedrock_names"]]
    assert sorted(bedrock.BEDROCK_MODELS) == names
    for name, row in zip(names, table["bedrock"]):
        for f, expected in zip(BEDROCK_FREQUENCIES, row):
            assert abs(complex(getattr(bedrock, name)(f)) - expected) <= 1e-12 * abs(expected), name
    assert complex(make_soil("flat", "bedrock_permittivity_granite_hartlieb16", temperature=270).permittivity(1.41e9)) == 5.45 + 0.038j


def test_permittivity_refusals_and_names():
    from smrt_amd.inputs.make_medium import get_permittivity_function, make_soil_substrate
    from smrt_amd.permittivity import soil

    with pytest.raises(SMRTError, match="above freezing"):
        soil.soil_permittivity_hut(10e9, 270.0, 0.2, 0.4, 0.3, 1100.0)
    with pytest.raises(SMRTError, match="above freezing"):
        soil.soil_permittivity_hut(10e9, np.array([280.0, 270.0]), 0.2, 0.4, 0.3, 1100.0)
    with pytest.raises(SMRTError, match="not implemented for above freezing"):
        soil.soil_permittivity_montpetit08(19e9, 274.0)
    assert make_soil is make_soil_substrate
    assert get_permittivity_function("soil_permittivity_hut") is soil.soil_permittivity_hut
    with pytest.warns(DeprecationWarning):
        assert get_permittivity_function("dobson85_peplinski95") is soil.soil_permittivity_dobson85_peplinski95
    for refused in ("dobson85", "soil_permittivity_dobson85"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with pytest.raises(SMRTError, match="outside the scope") as e:
                make_soil("flat", refused, 268.0, moisture=0.2, sand=0.4, clay=0.3)
        assert "soil_permittivity_dobson85_peplinski95" in str(e.value) and "soil_permittivity_dobson85_original" in str(e.value)
    with pytest.raises(SMRTError, match="valid name"):
        make_soil("flat", "nonsense", 268.0)
    # the default model is Dobson-Peplinski; a missing argument is named
    default = make_soil("soil_wegmuller", None, 270, moisture=0.2, sand=0.4, clay=0.3, roughness_rms=1e-2)
    assert default.permittivity_model is soil.soil_permittivity_dobson85_peplinski95 and default.moisture == 0.2 and default.temperature == 270
    with pytest.raises(SMRTError, match="Parameter sand must be specified"):
        make_soil("soil_wegmuller", "soil_permittivity_dobson85_peplinski95", 270, moisture=0.2, clay=0.3, roughness_rms=1e-2)
    with pytest.raises(SMRTError, match="Parameter roughness_rms must be specified"):
        make_soil("soil_wegmuller", "soil_permittivity_montpetit08", 270)
    # numbers and callables as before
    assert make_soil("flat", complex(5.0, 0.5), 270.0).device_params(1e9) == (5.0, 0.5)
    assert make_soil("flat", lambda f, t: 3 + 1e-10j * f, 270.0).device_params(1e9) == (3.0, 0.1)


def test_the_readme_example_builds():
    soil = make_soil("soil_wegmuller", "soil_permittivity_dobson85_peplinski95", 270, moisture=0.2, sand=0.4, clay=0.3,
                     dry_matter=1100, roughness_rms=1e-2)
    expected = load_golden("soil_wegmuller_dobson85_peplinski95")["eps_soil"]
    assert abs(soil.permittivity(37e9) - complex(expected)) <= 1e-12 * abs(expected)
    assert soil.device_kind == "soil_wegmuller" and soil.device_tail() == ((1e-2, 0.0), (0.0, 0.0))


# ---- the substrate protocol -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2], ids=["wegmuller", "qnh", "choudhury"])
def test_substrate_protocol_against_the_reference(k):
    g = load_golden("soil_edge")
    sub = edge_substrate(k)
    before = dict(vars(sub))
    for fi, f in enumerate(EDGE["frequency"]):
        mu, eps_last = g["mu_f%d_s%d" % (fi, k)], complex(g["eps_layers"][fi, k, -1])
        assert abs(sub.permittivity(f) - g["eps_soil"][fi, k]) <= 1e-12 * abs(g["eps_soil"][fi, k])
        for npol in (2, 3):
            spec, emis = sub.specular_reflection_matrix(f, eps_last, mu, npol), sub.emissivity_matrix(f, eps_last, mu, npol)
            assert spec.shape == emis.shape == (npol, len(mu))
            assert np.abs(spec - g["spec_f%d_s%d_npol%d" % (fi, k, npol)]).max() < 1e-13
            assert np.abs(emis - g["emis_f%d_s%d_npol%d" % (fi, k, npol)]).max() < 1e-13
    assert {a: repr(v) for a, v in vars(sub).items()} == {a: repr(v) for a, v in before.items()}   # (QNH: Nv, Nh untouched)


def test_qnh_defaults_stay_nan():
    sub = make_soil("soil_qnh", complex(6, 0.5), 270.0, H=0.3, N=1.0)
    sub.specular_reflection_matrix(19e9, 1.5 + 0j, np.array([0.9, 0.4]), 2)
    assert np.isnan(sub.Nv) and np.isnan(sub.Nh) and sub.device_tail() == ((0.3, 0.0), (1.0, 1.0))


# ---- packing ----------------------------------------------------------------------------------------------------------------
def test_packed_tails_hold_what_was_given():
    from smrt_amd.rtsolver.dort import DORT

    F, S = 2, 3
    subs = [make_soil("soil_qnh", "soil_permittivity_dobson85_original", 268.0 + s, moisture=0.1 + 0.05 * s, sand=0.5, clay=0.2,
                      H=0.3 + s, Q=0.1 * s, Nv=1.5 + s, Nh=0.5 * s) for s in range(S)]
    sps = [edge_snowpack(s, substrate=subs[s]) for s in range(S)]
    b = DORT(n_max_stream=8)._pack(sensor_list.passive(19e9, EDGE["theta"]), sps, np.array(EDGE["frequency"]), "iba")
    assert b.struct.substrate_kind == 5
    p1 = np.ctypeslib.as_array(b.struct.substrate_p1, (F * S + 2 * S,))
    p2 = np.ctypeslib.as_array(b.struct.substrate_p2, (F * S + 2 * S,))
    eps = np.array([[complex(sub.permittivity(f)) for sub in subs] for f in EDGE["frequency"]])
    # (evaluated on the columns of the group: the last bit of a vectorised power may differ from the scalar one)
    assert np.allclose(p1[:F * S].reshape(F, S), eps.real, rtol=1e-14, atol=0) and np.allclose(p2[:F * S].reshape(F, S), eps.imag, rtol=1e-14, atol=0)
    assert np.array_equal(p1[F * S:].reshape(S, 2), [[0.3 + s, 0.1 * s] for s in range(S)])
    assert np.array_equal(p2[F * S:].reshape(S, 2), [[1.5 + s, 0.5 * s] for s in range(S)])
    assert np.array_equal(np.ctypeslib.as_array(b.struct.substrate_temperature, (S,)), [268.0, 269.0, 270.0])
    # a named model is evaluated once per frequency on the columns of the group, not once per pair
    calls = []
    model = subs[0].permittivity_model

    def counting(frequency, **columns):
        calls.append(np.shape(columns["moisture"]))
        return model(frequency, **columns)
    counting.required_arguments, counting.optional_arguments = model.required_arguments, {}
    for sub in subs:
        sub.permittivity_model = counting
    DORT(n_max_stream=8)._pack(sensor_list.passive(19e9, EDGE["theta"]), sps, np.array(EDGE["frequency"]), "iba")
    assert calls == [(S,)] * F


def test_active_sensors_send_the_soils_down_the_host_route():
    from smrt_amd.core.snowpack import substrate_kind

    for k, code in enumerate((4, 5, 6)):
        sub = edge_substrate(k)
        assert substrate_kind(sub) == sub.device_kind and substrate_kind(sub, "A") == "host"
    from smrt_amd._native import PackedBatch

    with pytest.raises(SMRTError, match="passive mode only"):
        PackedBatch([1], [1.0], [0.3], [260.0], [1e-4], None, [19e9], [0.5], mode="A",
                    substrate=("soil_wegmuller", [[3.0]], [[0.1]], [270.0], [[1e-2, 0.0]], [[0.0, 0.0]]))


def test_active_dort_takes_the_protocol_route(emulated):
    model = make_model("iba", "dort", rtsolver_options=dict(n_max_stream=8, m_max=1))
    model.run(sensor_list.active(13e9, 35.0), edge_snowpack(0))
    probe_and_solve = [b for b, _ in emulated.batches]
    assert probe_and_solve[-1].struct.substrate_kind == 3 and probe_and_solve[-1].mode == "A"


def test_model_run_keeps_the_input_order_over_mixed_substrates(emulated):
    """no substrate, Flat, Wegmuller, QNH in one list: four device groups, the results where the inputs were."""
    flat = make_soil("flat", complex(6.0, 0.4), 268.0)
    packs = [edge_snowpack(2, substrate=None), edge_snowpack(1), edge_snowpack(0, substrate=flat), edge_snowpack(0),
             edge_snowpack(1, substrate=None), edge_snowpack(0)]
    model = make_model("iba", "dort", rtsolver_options=dict(n_max_stream=8))
    sensor = sensor_list.passive(EDGE["frequency"], EDGE["theta"])
    together = model.run(sensor, packs)
    assert sorted(int(b.struct.substrate_kind) for b, _ in emulated.batches) == [0, 1, 4, 5]
    g = load_golden("soil_edge")["dort_n8"]
    for i, sp in enumerate(packs):
        alone = model.run(sensor, sp)
        assert np.array_equal(np.asarray(together.TbV(snowpack=i)), np.asarray(alone.TbV()))
    for i, k in ((3, 0), (5, 0), (1, 1)):   # and the soil ones are the reference's
        tb = np.array([np.asarray(together.TbV(snowpack=i)), np.asarray(together.TbH(snowpack=i))])   # [pol][F][theta] or [pol][theta][F]
        tb = tb if tb.shape[1] == len(EDGE["frequency"]) else tb.transpose(0, 2, 1)
        assert np.abs(tb.transpose(1, 0, 2) - g[:, k]).max() < TB_ATOL


# ---- the device source under the emulators ----------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline,nt,order", PIPELINES)
def test_emulated_dort_on_the_wegmuller_cases(emu, pipeline, nt, order):
    from smrt_amd.rtsolver.dort import DORT

    for model, constants in WEGMULLER_CASES.items():
        expected = load_golden("soil_wegmuller_" + model[len("soil_permittivity_"):])["tb"]
        assert np.abs(expected - constants).max() < 1e-4   # (the reference's own constants, at its own bar)
        batch = DORT()._pack(sensor_list.passive(37e9, 40), [wegmuller_snowpack(model)], np.array([37e9]), "dmrt_qcacp_shortrange")
        assert batch.struct.substrate_kind == 4
        out, st = emu_run(emu, batch, pipeline, nt, order)
        assert st[0] == 0 and np.abs(out[0, :, 0] - expected).max() < TB_ATOL, (model, out[0, :, 0] - expected)


@pytest.mark.parametrize("pipeline,nt,order", PIPELINES)
def test_emulated_dort_on_soil_edge(emu, pipeline, nt, order):
    g = load_golden("soil_edge")["dort_n8"]
    batches, _ = pack_edge(8)
    for k, batch in enumerate(batches):
        assert batch.struct.substrate_kind == 4 + k
        out, st = emu_run(emu, batch, pipeline, nt, order)
        assert (st == 0).all() and np.abs(out - g[:, k]).max() < TB_ATOL, (k, np.abs(out - g[:, k]).max())


def test_emulated_dort_on_soil_edge_at_34_streams(emu):
    """N = 68: the smallest size on the eight-wavefront strip kernel (the emulator's pipeline 3 is the library's default there:
    global-workspace prep and diagonalisation, strip finish)."""
    g = load_golden("soil_edge")["dort_n34"]
    batches, _ = pack_edge(34)
    for k, batch in enumerate(batches):
        out, st = emu_run(emu, batch, 3, 256)
        assert (st == 0).all() and np.abs(out - g[:, k]).max() < TB_ATOL, (k, np.abs(out - g[:, k]).max())


@pytest.mark.parametrize("n_max_stream", [8, 34])
def test_successive_order_device_source_on_soil_edge(host_lib, n_max_stream):  # noqa: F811
    """Every order and the total against the reference's successive_order at 1e-6 K.  The reference's solver leaves the
    substrate's own emission out (the first documented difference of rtsolver/successive_order.py; with it this solver agrees
    with DORT, tests/test_successive_order_cpu.py::test_substrate_emission_against_dort): the soils of soil_edge emit 228 K
    at order 0 here and nothing there.  So the batch is handed over with substrate_temperature = 0 -- the soil reflects, as in
    the reference, and does not emit -- which compares the soil reflectivities of the kernel with the reference's, order by
    order; the emission term (1 - R) B(T) is the line the Flat substrate already had."""
    from smrt_amd.rtsolver.successive_order import SuccessiveOrder

    g = load_golden("soil_edge")["successive_order_n%d" % n_max_stream]
    batches, solver = pack_edge(n_max_stream, SuccessiveOrder, emitting=False, **EDGE_SO_OPTIONS)
    for k, batch in enumerate(batches):
        assert batch.struct.substrate_kind == 4 + k
        out = host_run(host_lib, batch, solver.n_iteration_max, solver.relative_tolerance)
        values = np.asarray(out.values).reshape(g[:, k].shape)
        assert (out.status == 0).all() and np.abs(values - g[:, k]).max() < TB_ATOL, (k, np.abs(values - g[:, k]).max())


def test_successive_order_with_emitting_soils_against_dort(host_lib):  # noqa: F811
    """The emitting soil in the successive-order kernel, which the reference's solver cannot check (it leaves the emission out):
    30 orders on the soil_edge snowpacks at 19 GHz against the reference's DORT on the same snowpacks and soils at the same 8
    streams.  Bar 0.5 K, the one tests/test_successive_order_cpu.py::test_substrate_emission_against_dort sets for a Flat
    substrate (twice the largest gap between the reference's own successive-order total and its DORT without a substrate);
    without the soil's emission the gap is above 100 K."""
    from smrt_amd.rtsolver.successive_order import SuccessiveOrder

    dort = load_golden("soil_edge")["dort_n8"][0]                 # [S][pol][theta] at 19 GHz
    cold = load_golden("soil_edge")["successive_order_n8"][0]     # the reference's successive_order: no emission from the soil
    batches, solver = pack_edge(8, SuccessiveOrder, n_iteration_max=30, relative_tolerance=0.0)
    for k, batch in enumerate(batches):
        out = host_run(host_lib, batch, 30, 0.0)
        total = np.asarray(out.values).reshape(2, 2, len(EDGE["theta"]), 31)[0, :, :, -1]
        gap = np.abs(total - dort[k]).max()
        print(f"successive_order (30 orders, emitting soil {k}) - DORT at 19 GHz: {gap:.4f} K; the reference's total without emission is "
              f"{np.abs(cold[k][:, :, -1] - dort[k]).min():.1f} K away")
        assert out.status[0] == 0 and gap < 0.5
        assert np.abs(cold[k][:, :, -1] - dort[k]).min() > 100.0


# ---- Choudhury out of its range ---------------------------------------------------------------------------------------------
def test_choudhury_out_of_range_is_an_error_or_nan_for_that_pair(emulated):
    rough = make_soil("rough_choudhury79", "soil_permittivity_montpetit08", 265.0, roughness_rms=2e-4)   # ksigma > 0.1 at 37 GHz only
    sensor = sensor_list.passive(EDGE["frequency"], EDGE["theta"])
    with pytest.raises(SMRTError, match="validity range"):
        make_model("iba", "dort", rtsolver_options=dict(n_max_stream=8)).run(sensor, edge_snowpack(2, substrate=rough))
    res = make_model("iba", "dort", rtsolver_options=dict(n_max_stream=8, error_handling="nan")).run(
        sensor, [edge_snowpack(2, substrate=rough), edge_snowpack(2)])
    tb = np.asarray(res.TbV())
    bad = np.isnan(tb)
    assert bad.sum() == len(EDGE["theta"]) and not np.isnan(np.asarray(res.TbV(snowpack=1))).any()
    assert np.isnan(np.asarray(res.TbV(snowpack=0, frequency=37e9))).all() and not np.isnan(np.asarray(res.TbV(snowpack=0, frequency=19e9))).any()
    with pytest.raises(SMRTError, match="validity range"):   # and on the host, as the reference raises
        rough.specular_reflection_matrix(37e9, 1.4 + 0j, np.array([0.8]), 2)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_multifresnel_keeps_refusing_non_flat_substrates():
    model = make_model("iba", "multifresnel_thermalemission")
    with pytest.raises(SMRTError, match="only works with flat substrates"):
        model.run(sensor_list.passive(19e9, 40.0), edge_snowpack(0))


def test_c_entry_points_refuse_as_specified(refusal):   # noqa: F811
    """The refusals of the C entry points through their CPU build (tests/hostemu/solver_refusals_host.cpp): the soil kinds need
    all three arrays, successive_order takes them, the multi-Fresnel solver answers with its flat-substrate message, the
    active solvers with theirs, and kinds above 6 are unknown to everyone."""
    arrays = dict(substrate_p1=True, substrate_p2=True, substrate_temperature=True)
    for kind in (4, 5, 6):
        assert refusal(SO, substrate_kind=kind, **arrays) is None
        for missing in arrays:
            assert refusal(SO, substrate_kind=kind, **dict(arrays, **{missing: None})) == "substrate arrays missing"
        assert refusal(MF, substrate_kind=kind, **arrays) == "the multi-Fresnel thermal emission solver takes no substrate or a Flat one"
        assert refusal(FO, substrate_kind=kind, **arrays) == FO_SUBSTRATE
        assert "takes no substrate or a flat one" in refusal(SOA, substrate_kind=kind, **arrays)
    assert refusal(SO, substrate_kind=7, **arrays) == "the successive_order solver takes no substrate, a flat one or a reflector"
    assert refusal(SO, substrate_kind=3, **arrays) == "the successive_order solver takes no substrate, a flat one or a reflector"


def test_dort_entry_point_refuses_as_specified(emu):
    """smrt_host::validate, the check of the DORT entry points, through the emulator (it validates before it runs)."""
    batches, _ = pack_edge(8)
    b = batches[0]

    def rc():
        n = b.n_pairs
        out, st = np.empty((n,) + b.out_shape()), np.empty(n, np.int32)
        return emu.smrt_emu_run(C.byref(b.struct), 0, n, 64, 0, out.ctypes.data_as(C.POINTER(C.c_double)),
                                st.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None)
    assert rc() == 0
    b.struct.substrate_temperature = None      # kinds 4 to 6 need all three arrays
    assert rc() != 0
    b.struct.substrate_temperature = b.sub_T.ctypes.data_as(C.POINTER(C.c_double))
    b.struct.substrate_kind = 7                # unknown above 6
    assert rc() != 0
    b.struct.substrate_kind = 4
    assert rc() == 0


# ---- the reference's own objects ----------------------------------------------------------------------------------------------
def test_reference_soil_objects_through_the_runner(smrt_ref, emulated):  # noqa: F811
    """Where the reference is present (skipped otherwise, like tests/test_reference_binding.py): its make_soil_substrate objects
    through HipBatchRunner are packed as device kind 4 and give the fixture's brightness temperatures."""
    smrt = smrt_ref
    from smrt.inputs.make_soil import make_soil_substrate as ref_make_soil

    from smrt_amd import HipBatchRunner

    spec, snow = EDGE["substrates"][0], EDGE["snow"][0]
    substrate = ref_make_soil(spec["model"], spec["permittivity_model"], spec["temperature"], **spec["soil"], **spec["parameters"])
    sp = smrt.make_snowpack(snow["thickness"], "exponential", density=snow["density"], temperature=snow["temperature"],
                            corr_length=snow["corr_length"], substrate=substrate)
    from smrt_amd.rtsolver.dort import DORT

    model = smrt.make_model("iba", DORT, rtsolver_options=dict(n_max_stream=8))
    res = model.run(smrt.sensor_list.passive(EDGE["frequency"], EDGE["theta"]), sp, runner=HipBatchRunner())
    assert [int(b.struct.substrate_kind) for b, _ in emulated.batches] == [4]
    g = load_golden("soil_edge")["dort_n8"][:, 0]
    dims = tuple(res.data.dims)   # (the stand-in of xarray has no .sel)
    tb = np.transpose(np.asarray(res.data.values, float), [dims.index(d) for d in ("frequency", "polarization", "theta")])
    assert np.abs(tb - g).max() < TB_ATOL
