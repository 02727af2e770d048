"""The successive-order solver on the GPU: every fixture through the C ABI and through Model.run at the project's bar for a
brightness temperature (1e-6 K, every order and the total, exact zeros where the fixture has them), one-shot against split
form, the substrate cases and a random batch against the NumPy restatement, batching into one launch per group, and the
chunking of the workspace under a small budget.

Layer scalars: eps 1e-12, ks 1e-11, ka 1e-10 relative (tests/test_gpu_first_order.py, tests/test_gpu_parity.py)."""
import os
import types

import numpy as np
import pytest

from smrt_amd import _native, make_model, sensor_list
from smrt_amd.core.error import SMRTError
from smrt_amd.inputs.make_medium import make_snowpack, make_soil
from smrt_amd.rtsolver.dort import get_context
from smrt_amd.rtsolver.successive_order import SuccessiveOrder
from successive_order_restatement import (FIXTURE_CASES, SUBSTRATE_CASES, TB_ATOL, build_snowpack, case_by_name, solve_case,
                                          solver_options, successive_order)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def api():
    from smrt_amd.substrate.reflector import make_reflector

    return types.SimpleNamespace(make_snowpack=make_snowpack, make_soil=make_soil, make_reflector=make_reflector)


def golden(case):
    return np.load(os.path.join(GOLDEN, "successive_order_" + case["name"] + ".npz"))


def assert_matches(values, reference, what):
    err = float(np.abs(values - reference).max())
    print(f"{what}: largest difference {err:.3e} K (bar {TB_ATOL:g})")
    assert np.array_equal(values == 0.0, reference == 0.0), what
    assert err <= TB_ATOL, (what, err)


def pack_case(case):
    solver = SuccessiveOrder(**solver_options(case))
    sensor = sensor_list.passive(case["frequency"], case["theta"])
    return solver._packer()._pack(sensor, [build_snowpack(case, api())], np.array([case["frequency"]]), case["emmodel"]), solver


@pytest.mark.parametrize("case", FIXTURE_CASES, ids=lambda c: c["name"])
def test_fixture_through_the_c_abi(case):
    g = golden(case)
    batch, solver = pack_case(case)
    out = get_context().successive_order_run(batch, solver.n_iteration_max, solver.relative_tolerance)
    assert out.status[0] == 0 and out.orders[0] == len(g["max_radiance"])
    assert_matches(out.values[0], g["tb"], "C ABI " + case["name"])
    L = len(case["thickness"])
    lay = out.layers[0][:L]
    assert np.abs(lay[:, 0] + 1j * lay[:, 1] - g["eps"]).max() <= 1e-12 * np.abs(g["eps"]).max()
    assert np.all(np.abs(lay[:, 2] - g["ks"]) <= 1e-11 * np.abs(g["ks"])) and np.all(np.abs(lay[:, 3] - g["ka"]) <= 1e-10 * np.abs(g["ka"]))
    assert np.array_equal(lay[:, 4].astype(int), g["streams"]) and np.array_equal(out.sublayers[0][:L], g["sublayers"])
    n = out.orders[0]
    assert np.abs(out.max_radiance[0][:n] / g["max_radiance"] - 1.0).max() < 1e-10 and np.all(out.max_radiance[0][n:] == 0.0)


@pytest.mark.parametrize("case", FIXTURE_CASES, ids=lambda c: c["name"])
def test_fixture_through_model_run(case):
    g = golden(case)
    m = make_model(case["emmodel"], "successive_order", rtsolver_options=solver_options(case))
    res = m.run(sensor_list.passive(case["frequency"], case["theta"]), build_snowpack(case, api()))
    assert res.data.dims == ("polarization", "theta", "order")
    assert_matches(res.data.values, g["tb"], "Model.run " + case["name"])
    assert abs(float(np.ravel(res.TbV(order="total"))[0]) - g["tb"][0, 0, -1]) <= TB_ATOL
    assert abs(float(np.ravel(res.TbH(order=0))[0]) - g["tb"][1, 0, 0]) <= TB_ATOL
    assert np.all(np.abs(res.other_data["ks"].values - g["ks"]) <= 1e-11 * np.abs(g["ks"]))


def test_one_shot_and_split_form_agree():
    case = case_by_name("iba_refraction_L3_n6")
    batch, solver = pack_case(case)
    ctx = get_context()
    one = ctx.successive_order_run(batch, solver.n_iteration_max, solver.relative_tolerance)
    with ctx.lock:
        ctx.successive_order_upload(batch, solver.n_iteration_max, solver.relative_tolerance)
        ctx.successive_order_launch()
        ctx.successive_order_sync()
        prep_ms, sweep_ms = ctx.successive_order_kernel_ms()
        two = ctx.successive_order_download()
    for name in ("raw", "status", "layers", "streams", "sublayers", "max_radiance", "orders"):
        assert np.array_equal(getattr(one, name), getattr(two, name)), name
    assert prep_ms > 0.0 and sweep_ms > 0.0


@pytest.mark.parametrize("case", SUBSTRATE_CASES, ids=lambda c: c["name"])
def test_substrate_cases_against_the_restatement(case):
    sol, _ = solve_case(case)
    m = make_model(case["emmodel"], "successive_order", rtsolver_options=solver_options(case))
    res = m.run(sensor_list.passive(case["frequency"], case["theta"]), build_snowpack(case, api()))
    assert_matches(res.data.values, sol["tb"], "Model.run " + case["name"])


# ---- a random batch: 64 snowpacks of 2 to 6 layers, 8 streams, 2 frequencies ---------------------------------------------
FREQUENCIES = [19e9, 37e9]
OPTIONS = dict(n_max_stream=8, n_iteration_max=10)
DEEP = 17   # index of the snowpack made optically very deep for the chunking test


def random_columns(deep=False):
    rng = np.random.RandomState(20261017)
    cols = []
    for k in range(64):
        L = int(rng.randint(2, 7))
        c = dict(thickness=list(rng.uniform(0.05, 0.6, L)), density=list(rng.uniform(150.0, 450.0, L)),
                 temperature=list(rng.uniform(245.0, 270.0, L)), corr_length=list(rng.uniform(5e-5, 3e-4, L)))
        c["thickness"][-1] = float(rng.uniform(0.5, 8.0))
        if deep and k == DEEP:
            c["thickness"][-1] = 20000.0
        cols.append(c)
    return cols


@pytest.fixture(scope="module")
def random_batch():
    """(columns, snowpacks, restatement [F, S, 2, 1, orders + 1], orders run [F, S]) -- computed once, never modified."""
    from oracle import dort_oracle as O

    cols = random_columns()
    sps = [make_snowpack(c["thickness"], "exponential", density=c["density"], temperature=c["temperature"], corr_length=c["corr_length"])
           for c in cols]
    ref = np.empty((2, 64, 2, 1, OPTIONS["n_iteration_max"] + 1))
    orders = np.empty((2, 64), int)
    for f, frequency in enumerate(FREQUENCIES):
        for s, c in enumerate(cols):
            sp = dict(thickness=np.array(c["thickness"]), density=np.array(c["density"]), temperature=np.array(c["temperature"]),
                      microstructure="exponential", corr_length=np.array(c["corr_length"]))
            sol = successive_order(O.make_layers("iba", frequency, sp), c["thickness"], c["temperature"], frequency, [53.0], **OPTIONS)
            ref[f, s], orders[f, s] = sol["tb"], sol["orders"]
    return cols, sps, ref, orders


def test_batch_against_the_restatement_in_one_launch(random_batch):
    cols, sps, ref, orders = random_batch
    m = make_model("iba", "successive_order", rtsolver_options=OPTIONS)
    solver = SuccessiveOrder(**OPTIONS)
    res = solver.solve_plan(m, m.plan(sensor_list.passive(FREQUENCIES, 53), sps))
    assert solver.launches == 1 and solver.launch_info[0]["chunks"] == 1
    assert res.data.dims == ("frequency", "snowpack", "polarization", "theta", "order")
    assert_matches(res.data.values, ref, "batch of 64 x 2")
    assert len(np.unique(orders)) > 1, "the pairs must stop at different orders"
    stopped = (res.data.values[:, :, 0, 0, :-1] != 0.0).sum(axis=-1)
    assert np.array_equal(stopped, orders)
    for f, s in ((0, 3), (1, 40), (1, DEEP)):   # each result is bitwise the single solve of the same simulation
        single = m.run(sensor_list.passive(FREQUENCIES[f], 53), sps[s])
        assert np.array_equal(single.data.values, res.data.values[f, s])


def test_launch_counter_through_solve_batch(random_batch):
    cols, sps, ref, orders = random_batch
    soil = make_soil("flat", complex(3.0, 0.1), 265.0)
    c = cols[0]
    with_soil = make_snowpack(c["thickness"], "exponential", density=c["density"], temperature=c["temperature"],
                              corr_length=c["corr_length"], substrate=soil)
    solver = SuccessiveOrder(**OPTIONS)
    sensors = [sensor_list.passive(f, 53) for f in FREQUENCIES]
    sims = [(sensor, sp) for sensor in sensors for sp in sps[:8] + [with_soil]]
    results = solver.solve_batch(sims, "iba")
    assert solver.launches == 2 and len(results) == 18   # one group without substrate, one on soil
    for k in range(8):
        assert np.abs(results[k].data.values - ref[0, k]).max() <= TB_ATOL
    assert np.all(np.isfinite(results[8].data.values))


def test_chunking_under_a_small_budget(random_batch):
    cols, sps, ref, orders = random_batch
    deep_cols = random_columns(deep=True)
    c = deep_cols[DEEP]
    deep_sps = list(sps)
    deep_sps[DEEP] = make_snowpack(c["thickness"], "exponential", density=c["density"], temperature=c["temperature"],
                                   corr_length=c["corr_length"])
    budget = 2 << 20
    batch = SuccessiveOrder(**OPTIONS)._packer()._pack(sensor_list.passive(FREQUENCIES[0], 53), deep_sps, np.array(FREQUENCIES), "iba")
    ctx = get_context()
    with ctx.lock:
        out = ctx.successive_order_run(batch, OPTIONS["n_iteration_max"], 0.001, workspace_budget=budget)
        info = ctx.successive_order_launch_info()
    assert info["chunks"] > 2 and info["reserved_bytes"] <= budget and info["over_budget"] == 2
    flat_ref = ref.reshape(128, 2, 1, -1)
    deep_rows = [DEEP, 64 + DEEP]
    assert list(np.nonzero(out.status)[0]) == deep_rows and np.all(out.status[deep_rows] == 7)
    assert np.all(np.isnan(out.values[deep_rows]))
    ok = np.setdiff1d(np.arange(128), deep_rows)
    whole = ctx.successive_order_run(batch, OPTIONS["n_iteration_max"], 0.001, pairs=ok)
    assert np.array_equal(whole.raw, out.raw[ok]), "the chunked launch must give the bits of the unchunked one"
    assert_matches(out.values[ok], flat_ref[ok], "chunked batch")
    with pytest.raises(SMRTError, match="optically too deep for the successive_order workspace: [0-9]+ sublayers"):
        SuccessiveOrder(**dict(OPTIONS, workspace_budget=budget)).solve_batch([(sensor_list.passive(37e9, 53), deep_sps[DEEP])], "iba")
    with pytest.raises(SMRTError, match="budget"):
        ctx.successive_order_run(batch, OPTIONS["n_iteration_max"], 0.001, workspace_budget=1024)
