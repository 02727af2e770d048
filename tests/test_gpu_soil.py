"""Soil substrates (Wegmuller, QNH, Choudhury) on the GPU: the reference's brightness temperatures of the soil fixtures
(tests/golden/make_soil_fixtures.py) through Model.run on the default pipeline (N <= 64: the strip finish kernel on four
wavefronts, its SOIL instance), with the register-resident finish kernel (set_pipeline(3)), the two-slot (4) and four-slot (2)
finish kernels and the fused kernel (0), through successive_order, at the sizes where the code takes another path
(n_max_stream 34: N = 68, the smallest size on the eight-wavefront strip kernel; 66: N = 132, the smallest on the big
global-workspace pipeline), and the device route against the dense host route of the same objects on a random batch.

Bars: 1e-6 K against the reference (the package's contract); 2e-6 K between the two routes, each of which is held to 1e-6 K
against the reference.  Every test prints the largest difference it saw (profiles/soil_parity.txt)."""
import numpy as np
import pytest

from conftest import load_golden
from soil_cases import EDGE, EDGE_SO_OPTIONS, WEGMULLER_CASES
from test_soil_cpu import edge_snowpack, pack_edge, wegmuller_snowpack

from smrt_amd import make_model, make_soil, sensor_list
from smrt_amd.rtsolver.dort import get_context

pytestmark = pytest.mark.gpu

TB_ATOL = 1e-6
ROUTES_ATOL = 2e-6


def edge_tb(res, n_snowpacks=3):
    """[F][S][pol][theta] of a Model.run over the snowpacks of soil_edge and its two frequencies."""
    return np.array([[[np.asarray(res.TbV(frequency=f, snowpack=s)), np.asarray(res.TbH(frequency=f, snowpack=s))]
                      for s in range(n_snowpacks)] for f in EDGE["frequency"]])


def run_edge(n_max_stream, pipeline=1):
    ctx = get_context()
    ctx.set_pipeline(pipeline)
    try:
        model = make_model("iba", "dort", rtsolver_options=dict(n_max_stream=n_max_stream))
        return edge_tb(model.run(sensor_list.passive(EDGE["frequency"], EDGE["theta"]), [edge_snowpack(k) for k in range(3)]))
    finally:
        ctx.set_pipeline(1)


@pytest.mark.parametrize("pipeline", [1, 3])
def test_wegmuller_cases_of_the_reference(pipeline):
    ctx = get_context()
    ctx.set_pipeline(pipeline)
    try:
        for model, constants in WEGMULLER_CASES.items():
            expected = load_golden("soil_wegmuller_" + model[len("soil_permittivity_"):])["tb"]
            res = make_model("dmrt_qcacp_shortrange", "dort").run(sensor_list.passive(37e9, 40), wegmuller_snowpack(model))
            tb = np.array([float(res.TbV()), float(res.TbH())])
            print(f"soil_wegmuller {model} pipeline {pipeline}: largest difference {np.abs(tb - expected).max():.3e} K")
            assert np.abs(tb - expected).max() < TB_ATOL and np.abs(tb - constants).max() < 1e-4
    finally:
        ctx.set_pipeline(1)


@pytest.mark.parametrize("n_max_stream,pipeline,kernels", [(8, 1, "lds_strip"), (8, 3, "lds_reg"), (8, 4, "lds_two_slot"), (8, 2, "lds_four_slot"),
                                                           (8, 0, "fused"), (34, 1, "gmem_strip"), (66, 1, "big")])
def test_soil_edge_through_model_run(n_max_stream, pipeline, kernels):
    """... on the pipeline a Flat substrate gets: the dispatcher does not move a soil batch elsewhere."""
    expected = load_golden("soil_edge")["dort_n%d" % n_max_stream]
    tb = run_edge(n_max_stream, pipeline)
    ctx = get_context()
    ctx.set_pipeline(pipeline)
    try:
        for batch in pack_edge(n_max_stream)[0]:
            ctx.upload(batch)
            assert ctx.launch_info()["pipeline"] == kernels, ctx.launch_info()
    finally:
        ctx.set_pipeline(1)
    err = np.abs(tb - expected).max(axis=(0, 2, 3))
    print(f"soil_edge n_max_stream {n_max_stream} pipeline {pipeline}: largest difference (Wegmuller, QNH, Choudhury) {err} K")
    assert err.max() < TB_ATOL


def test_soil_edge_through_successive_order():
    """Every order and the total against the reference's successive_order.  The reference's solver leaves the substrate's own
    emission out (tests/test_soil_cpu.py::test_successive_order_device_source_on_soil_edge), so the packed batches are launched
    with substrate_temperature = 0: the soils reflect, as in the reference, and do not emit."""
    from smrt_amd.rtsolver.successive_order import SuccessiveOrder

    expected = load_golden("soil_edge")["successive_order_n8"]
    batches, solver = pack_edge(8, SuccessiveOrder, emitting=False, **EDGE_SO_OPTIONS)
    for k, batch in enumerate(batches):
        out = get_context().successive_order_run(batch, solver.n_iteration_max, solver.relative_tolerance)
        values = np.asarray(out.values).reshape(expected[:, k].shape)
        err = np.abs(values - expected[:, k]).max()
        print(f"soil_edge successive_order substrate {k}: largest difference over the orders and the total {err:.3e} K")
        assert (out.status == 0).all() and err < TB_ATOL
    # and through Model.run with the emitting soils: finite, and warmer than the non-emitting answer of the reference
    model = make_model("iba", "successive_order", rtsolver_options=dict(n_max_stream=8, **EDGE_SO_OPTIONS))
    res = model.run(sensor_list.passive(EDGE["frequency"][1], EDGE["theta"]), [edge_snowpack(k) for k in range(3)])
    total = np.asarray(res.TbV(order="total"))
    assert np.isfinite(total).all() and (total.reshape(3, -1) > expected[1, :, 0, :, -1]).all()


class HostRoute:
    """The same substrate object without its device_kind: the dense host route (SMRT_SUBSTRATE_HOST) evaluates it."""

    def __init__(self, substrate):
        self.substrate, self.temperature = substrate, substrate.temperature

    def specular_reflection_matrix(self, *args):
        return self.substrate.specular_reflection_matrix(*args)

    def emissivity_matrix(self, *args):
        return self.substrate.emissivity_matrix(*args)


def test_device_route_against_the_dense_host_route_on_random_wegmuller_soils():
    rng = np.random.default_rng(1999)
    soils = [make_soil("soil_wegmuller", "soil_permittivity_dobson85_peplinski95", rng.uniform(262, 273), moisture=rng.uniform(0.05, 0.35),
                       sand=rng.uniform(0.2, 0.6), clay=rng.uniform(0.1, 0.3), roughness_rms=rng.uniform(2e-3, 2e-2)) for _ in range(64)]
    snow = [dict(thickness=[rng.uniform(0.1, 0.5), rng.uniform(0.2, 0.8)], density=[rng.uniform(330, 420), rng.uniform(180, 260)],
                 temperature=[rng.uniform(245, 265), rng.uniform(250, 268)], corr_length=[rng.uniform(5e-5, 2e-4), rng.uniform(1e-4, 3e-4)])
            for _ in range(64)]
    from smrt_amd import make_snowpack

    def packs(wrap):
        return [make_snowpack(s["thickness"], "exponential", density=s["density"], temperature=s["temperature"],
                              corr_length=s["corr_length"], substrate=wrap(soil)) for s, soil in zip(snow, soils)]
    model = make_model("iba", "dort", rtsolver_options=dict(n_max_stream=8))
    sensor = sensor_list.passive(EDGE["frequency"], EDGE["theta"])
    device = edge_tb(model.run(sensor, packs(lambda soil: soil)), 64)
    host = edge_tb(model.run(sensor, packs(HostRoute)), 64)
    print(f"64 random snow-on-Wegmuller snowpacks, device route against dense host route: largest difference {np.abs(device - host).max():.3e} K")
    assert np.isfinite(device).all() and np.abs(device - host).max() < ROUTES_ATOL
