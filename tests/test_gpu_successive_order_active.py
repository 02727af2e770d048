"""The successive-order backscatter solver on the GPU: every fixture through the C ABI and through Model.run, one-shot
against split form, a ragged random batch and the column counts 1 to 12 against the NumPy restatement, batching into one
launch per group, and the chunking of the workspace under a small budget.

Bar: every element (each order and the total, all nine polarisation pairs) within 1e-8 x the largest co-polarised total of
the fixture / of the pair (profiles/first_order_parity.txt), exact zeros exactly where the reference has them.
Layer scalars: eps 1e-12, ks 1e-11, ka 1e-10 relative (tests/test_gpu_parity.py)."""
import os
import types

import numpy as np
import pytest

from smrt_amd import make_model, sensor_list
from smrt_amd.core.error import SMRTError
from smrt_amd.inputs.make_medium import make_snowpack, make_soil
from smrt_amd.rtsolver.dort import get_context
from smrt_amd.rtsolver.successive_order_backscatter import SuccessiveOrderBackscatter
from successive_order_active_restatement import (CASES, PARITY_RTOL, build_snowpack, case_by_name, parity_bar, solver_options,
                                                 successive_order_backscatter)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def api():
    return types.SimpleNamespace(make_snowpack=make_snowpack, make_soil=make_soil)


def golden(case):
    return np.load(os.path.join(GOLDEN, "successive_order_active_" + case["name"] + ".npz"))


def assert_matches(values, reference, what):
    """One pair: [3, 3, n_theta_inc, orders + 1]."""
    bar = parity_bar(reference)
    err = float(np.abs(values - reference).max())
    print(f"{what}: largest difference {err:.3e} = {err / bar * PARITY_RTOL:.2e} x the largest co-polarised total (bar 1e-8)")
    assert np.array_equal(values == 0.0, reference == 0.0), what
    assert err <= bar, (what, err, bar)


def pack_case(case):
    solver = SuccessiveOrderBackscatter(**solver_options(case))
    sensor = sensor_list.active(case["frequency"], case["theta"])
    batch = solver._packer()._pack(sensor, [build_snowpack(case, api())], np.array([case["frequency"]]), case["emmodel"])
    return batch, solver, sensor


def run_args(solver, sensor):
    return (np.atleast_1d(sensor.theta_inc), solver.n_iteration_max, solver.relative_tolerance), \
        dict(incident_npol=len(solver.incident_polarizations), m_max=solver.m_max)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_fixture_through_the_c_abi(case):
    g = golden(case)
    batch, solver, sensor = pack_case(case)
    args, kw = run_args(solver, sensor)
    out = get_context().so_active_run(batch, *args, **kw)
    assert out.status[0] == 0
    assert_matches(out.values[0], g["sigma"], "C ABI " + case["name"])
    L = len(case["thickness"])
    lay = out.layers[0][:L]
    assert np.abs(lay[:, 0] + 1j * lay[:, 1] - g["eps"]).max() <= 1e-12 * np.abs(g["eps"]).max()
    assert np.all(np.abs(lay[:, 2] - g["ks"]) <= 1e-11 * np.abs(g["ks"])) and np.all(np.abs(lay[:, 3] - g["ka"]) <= 1e-10 * np.abs(g["ka"]))
    assert np.array_equal(lay[:, 4].astype(int), g["streams"]) and np.array_equal(out.sublayers[0][:L], g["sublayers"])
    ran = ~np.isnan(g["pass_max"])
    assert np.array_equal(np.isnan(out.max_radiance[0]), ~ran) and np.array_equal(out.orders[0], ran.sum(axis=1))
    assert np.all(np.abs(out.max_radiance[0][ran] - g["pass_max"][ran]) <= 1e-10 * np.abs(g["pass_max"][ran]))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_fixture_through_model_run(case):
    g = golden(case)
    m = make_model(case["emmodel"], "successive_order_backscatter", rtsolver_options=solver_options(case))
    res = m.run(sensor_list.active(case["frequency"], case["theta"]), build_snowpack(case, api()))
    assert res.data.dims == ("polarization_inc", "polarization", "theta_inc", "order")
    assert_matches(np.asarray(res.data.values), g["sigma"], "Model.run " + case["name"])
    scale = 4 * np.pi * np.cos(np.deg2rad(case["theta"]))
    assert np.abs(np.ravel(res.sigmaVV(order="total")) - scale * g["sigma"][0, 0, :, -1]).max() <= parity_bar(g["sigma"]) * scale.max()
    assert np.all(np.abs(res.other_data["ks"].values - g["ks"]) <= 1e-11 * np.abs(g["ks"]))


def test_one_shot_and_split_form_agree():
    batch, solver, sensor = pack_case(case_by_name("iba_refraction_L3_n6"))
    args, kw = run_args(solver, sensor)
    ctx = get_context()
    one = ctx.so_active_run(batch, *args, **kw)
    with ctx.lock:
        ctx.so_active_upload(batch, *args, **kw)
        ctx.so_active_launch()
        ctx.so_active_sync()
        prep_ms, sweep_ms, combine_ms = ctx.so_active_kernel_ms()
        two = ctx.so_active_download()
    for name in ("values", "status", "layers", "streams", "sublayers", "max_radiance", "orders"):
        assert np.array_equal(getattr(one, name), getattr(two, name), equal_nan=name == "max_radiance"), name
    assert prep_ms > 0.0 and sweep_ms > 0.0 and combine_ms > 0.0


# ---- a ragged random batch: 24 snowpacks of 1 to 4 layers x 2 frequencies, 8 streams, 2 angles, 6 orders ----------------------
FREQUENCIES = [13e9, 17e9]
ANGLES = [30.0, 50.0]
OPTIONS = dict(n_max_stream=8, n_iteration_max=6)
SOIL = 5    # index of the snowpack on a Flat soil
DEEP = 11   # index of the snowpack made optically very deep for the chunking test
SOIL_EPS = complex(5.0, 0.5)


def random_columns(deep=False):
    rng = np.random.RandomState(20261018)
    cols = []
    for k in range(24):
        L = int(rng.randint(1, 5))
        c = dict(thickness=list(rng.uniform(0.05, 0.6, L)), density=list(rng.uniform(150.0, 450.0, L)),
                 temperature=list(rng.uniform(245.0, 270.0, L)), corr_length=list(rng.uniform(1e-4, 6e-4, L)))
        c["thickness"][-1] = float(rng.uniform(0.5, 4.0))
        if deep and k == DEEP:
            c["thickness"][-1] = 20000.0
        cols.append(c)
    return cols


def snowpack_of(c, soil=False):
    return make_snowpack(c["thickness"], "exponential", density=c["density"], temperature=c["temperature"], corr_length=c["corr_length"],
                         substrate=make_soil("flat", SOIL_EPS, 265.0) if soil else None)


def restate(c, frequency, theta, soil=False, **options):
    from oracle import dort_oracle as O

    sp = dict(thickness=np.array(c["thickness"]), density=np.array(c["density"]), temperature=np.array(c["temperature"]),
              microstructure="exponential", corr_length=np.array(c["corr_length"]))
    return successive_order_backscatter(O.make_layers("iba", frequency, sp), c["thickness"], theta,
                                        substrate=dict(kind="flat", eps=SOIL_EPS) if soil else None, **options)


@pytest.fixture(scope="module")
def random_batch():
    """(columns, snowpacks, restatement [F, S, 3, 3, 2, orders + 1]) -- computed once, never modified."""
    cols = random_columns()
    sps = [snowpack_of(c, soil=k == SOIL) for k, c in enumerate(cols)]
    ref = np.empty((2, 24, 3, 3, 2, OPTIONS["n_iteration_max"] + 1))
    for f, frequency in enumerate(FREQUENCIES):
        for s, c in enumerate(cols):
            ref[f, s] = restate(c, frequency, ANGLES, soil=s == SOIL, **OPTIONS)["sigma"]
    return cols, sps, ref


def test_batch_against_the_restatement_in_one_launch_per_group(random_batch):
    cols, sps, ref = random_batch
    m = make_model("iba", "successive_order_backscatter", rtsolver_options=OPTIONS)
    solver = SuccessiveOrderBackscatter(**OPTIONS)
    res = solver.solve_plan(m, m.plan(sensor_list.active(FREQUENCIES, ANGLES), sps))
    assert solver.launches == 2 and all(info["chunks"] == 1 for info in solver.launch_info)   # without substrate; on soil
    assert res.data.dims == ("frequency", "snowpack", "polarization_inc", "polarization", "theta_inc", "order")
    values = np.asarray(res.data.values)
    for f in range(2):
        for s in range(24):
            assert_matches(values[f, s], ref[f, s], f"batch, frequency {f}, snowpack {s}")
    plain = [sp for k, sp in enumerate(sps) if k != SOIL]
    res = solver.solve_plan(m, m.plan(sensor_list.active(FREQUENCIES, ANGLES), plain))
    assert solver.launches == 1 and solver.launch_info[0]["chunks"] == 1
    assert np.array_equal(np.asarray(res.data.values), np.delete(values, SOIL, axis=1)), "one launch gives the bits of two"
    single = m.run(sensor_list.active(FREQUENCIES[1], ANGLES), sps[3])
    assert np.array_equal(np.asarray(single.data.values), values[1, 3])


@pytest.mark.parametrize("columns, theta, pols", [(1, [85.0], "V"), (2, [40.0], "V"), (3, [85.0], "VHU"), (4, [40.0], "VH"),
                                                  (6, [40.0], "VHU"), (8, [15.0, 55.0], "VH"), (12, [15.0, 55.0], "VHU")])
def test_column_counts_against_the_restatement(columns, theta, pols):
    """Tile-row padding of the flattened (sublayer, column) dimension: 2 layers of 1 and 4 sublayers, C columns."""
    c = dict(thickness=[0.2, 0.5], density=[250.0, 350.0], temperature=[255.0, 262.0], corr_length=[2e-4, 6e-4])
    options = dict(n_max_stream=8, n_iteration_max=4, incident_polarizations=pols)
    sol = restate(c, 13e9, theta, **options)
    assert sol["columns"] == columns and list(sol["sublayers"]) == [1, 4]
    m = make_model("iba", "successive_order_backscatter", rtsolver_options=options)
    res = m.run(sensor_list.active(13e9, theta), snowpack_of(c))
    assert_matches(np.asarray(res.data.values), sol["sigma"], f"{columns} columns")


def test_chunking_under_a_small_budget(random_batch):
    cols, sps, ref = random_batch
    c = random_columns(deep=True)[DEEP]
    plain = [k for k in range(24) if k != SOIL]
    deep_sps = [snowpack_of(c) if k == DEEP else sps[k] for k in plain]
    row = plain.index(DEEP)
    budget = 3 << 20
    solver = SuccessiveOrderBackscatter(**OPTIONS)
    sensor = sensor_list.active(FREQUENCIES[0], ANGLES)
    batch = solver._packer()._pack(sensor, deep_sps, np.array(FREQUENCIES), "iba")
    args, kw = run_args(solver, sensor)
    ctx = get_context()
    with ctx.lock:
        out = ctx.so_active_run(batch, *args, workspace_budget=budget, **kw)
        info = ctx.so_active_launch_info()
    assert info["chunks"] > 1 and info["reserved_bytes"] <= budget and info["over_budget"] == 2
    deep_rows = [row, 23 + row]
    assert list(np.nonzero(out.status)[0]) == deep_rows and np.all(out.status[deep_rows] == 7)
    assert np.all(np.isnan(out.values[deep_rows]))
    ok = np.setdiff1d(np.arange(46), deep_rows)
    whole = ctx.so_active_run(batch, *args, pairs=ok, **kw)
    assert np.array_equal(whole.values, out.values[ok]), "the chunked launch must give the bits of the unchunked one"
    flat_ref = ref[:, plain].reshape(46, 3, 3, 2, -1)
    for k in ok:
        assert_matches(out.values[k], flat_ref[k], f"chunked batch, row {k}")
    with pytest.raises(SMRTError, match="optically too deep for the successive_order workspace: [0-9]+ sublayers"):
        SuccessiveOrderBackscatter(**dict(OPTIONS, workspace_budget=budget)).solve_batch([(sensor, deep_sps[row])], "iba")
    with pytest.raises(SMRTError, match="budget"):
        ctx.so_active_run(batch, *args, workspace_budget=1024, **kw)
