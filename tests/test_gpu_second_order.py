"""The iterative second-order solver on the GPU: every fixture through the C ABI and through Model.run, a batch of 70 pairs
that mixes layer counts (padding, more than one wavefront of units) against the NumPy restatement with the interlayer term
off and on, the split form against the one shot, and the first-order contributions against `iterative_first_order`.

Tolerance: SIGMA_RTOL = 1e-8 of the solve's largest co-polarised total (tests/test_second_order_cpu.py)."""
import numpy as np
import pytest

import test_second_order_cpu as T
from second_order_restatement import CASES, CONTRIBUTIONS, build_snowpack, options_of, solve_case
from smrt_amd import _native, make_model, sensor_list

pytestmark = pytest.mark.gpu
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def ctx():
    from smrt_amd.rtsolver.dort import get_context

    return get_context(None)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture_through_the_c_abi(case, ctx):
    out = T.run_case(case, ctx)
    assert out.status[0] == 0
    L = len(case["thickness"])
    g = T.golden(case)
    T.assert_close(case["name"], case["theta"], out.values[0], out.layer_backscatter[0][:L + 1], g["contributions"], g["backscatter_layer"], "C ABI")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture_through_model_run(case):
    sp = build_snowpack(case, T.api())
    model = make_model(case["emmodel"], "iterative_second_order", rtsolver_options=dict(return_contributions=True, **options_of(case)))
    res = model.run(sensor_list.active(case["frequency"], case["theta"]), sp)
    assert list(res.data.dims) == ["contribution", "theta_inc", "polarization_inc", "polarization"]
    assert list(res.data.coords["contribution"]) == CONTRIBUTIONS and list(res.data.coords["polarization"]) == ["V", "H"]
    data = np.asarray(res.data.values, float)
    g = T.golden(case)
    T.assert_close(case["name"], case["theta"], data[1:], np.asarray(res.other_data["backscatter_layer"].values, float), g["contributions"],
                   g["backscatter_layer"], "Model.run")
    assert np.array_equal(data[0], data[1] + data[2] + data[3] + data[4] + data[5] + data[6] + data[7])
    total = make_model(case["emmodel"], "iterative_second_order", rtsolver_options=options_of(case)).run(
        sensor_list.active(case["frequency"], case["theta"]), sp)
    assert list(total.data.dims) == ["theta_inc", "polarization_inc", "polarization"] and np.array_equal(np.asarray(total.data.values), data[0])


@pytest.fixture(scope="module")
def batch70():
    rng = np.random.RandomState(5)
    return T.random_batch(rng, [1, 2, 3, 5] * 17 + [3, 1], [20.0, 35.0, 50.0], n_max_stream=6, m_max=3)


@pytest.mark.parametrize("interlayer", [False, True], ids=["plain", "interlayer"])
def test_batch_of_70_pairs_matches_the_restatement(batch70, ctx, interlayer):
    out, sps = T.solve_batch_on(ctx, batch70, interlayer)
    assert len(batch70) == 70 and not out.status.any()
    worst = 0.0
    for k, (case, sp) in enumerate(zip(batch70, sps)):
        (c, pl), _ = solve_case(dict(case, interlayer=interlayer), sp)
        L = len(case["thickness"])
        worst = max(worst, T.assert_close(case["name"], case["theta"], out.values[k], out.layer_backscatter[k][:L + 1],
                                          np.concatenate([c.sum(axis=0)[None], c]), pl, "GPU"))
        assert not out.layer_backscatter[k][L + 1:].any()
    print("worst of the batch:", worst)


def pack_batch(cases, interlayer, budget=None):
    from smrt_amd import _native
    from smrt_amd.core.model import SimulationPlan
    from smrt_amd.rtsolver.iterative_second_order import IterativeSecondOrder

    sps = [build_snowpack(c, T.api()) for c in cases]
    sensor = sensor_list.active(cases[0]["frequency"], cases[0]["theta"])
    solver = IterativeSecondOrder(n_max_stream=cases[0]["n_max_stream"], m_max=cases[0]["m_max"])
    packer = solver._packer()
    names = solver.emmodel_names(make_model("iba", "iterative_second_order"),
                                 SimulationPlan([sensor], sps, np.zeros(len(sps), int), np.arange(len(sps))))
    batch = packer._pack(sensor, sps, np.array([float(cases[0]["frequency"])]), names, {})
    return batch, _native.PackedSecondOrderExtras(batch, interlayer, budget)


def test_split_form_equals_the_one_shot_bit_for_bit(batch70, ctx):
    batch, extras = pack_batch(batch70, True)
    one = ctx.second_order_run(batch, extras)
    with ctx.lock:
        ctx.second_order_upload(batch, extras)
        ctx.second_order_launch()
        ctx.second_order_launch()
        ctx.second_order_sync()
        two = ctx.second_order_download()
    for name in ("values", "status", "layers", "layer_backscatter", "diag"):
        assert np.array_equal(getattr(one, name), getattr(two, name)), name
    assert all(ms > 0 for ms in ctx.second_order_kernel_ms())
    # a budget that forces several chunks of pairs gives the same bits, listed pairs too
    fixed = 70 * (5 * 3 * 5 + 28 * 3 + 6 * 3 * 4) * 8 + 6 * 8
    per_row = 5 * 4 + 5 * 2 * 6 * 8 + 5 * 3 * 7 * 4 * 8
    small = ctx.second_order_run(batch, pack_batch(batch70, True, budget=fixed + 9 * per_row)[1])
    assert np.array_equal(one.values, small.values) and np.array_equal(one.layer_backscatter, small.layer_backscatter)
    some = ctx.second_order_run(batch, extras, pairs=[69, 3, 3, 40])
    assert np.array_equal(some.values, one.values[[69, 3, 3, 40]])


def test_first_order_contributions_are_those_of_the_first_order_solver(batch70, ctx):
    batch, extras = pack_batch(batch70, False)
    second = ctx.second_order_run(batch, extras)
    first = ctx.first_order_run(batch)
    assert np.array_equal(second.values[:, :4], first.values)
    assert np.array_equal(second.layers, first.layers) and np.array_equal(second.diag, first.diag)
    sps = [build_snowpack(c, T.api()) for c in batch70[:8]]
    sensor = sensor_list.active(13e9, [20.0, 35.0, 50.0])
    opts = dict(return_contributions=True)
    r1 = make_model("iba", "iterative_first_order", rtsolver_options=opts).run(sensor, sps)
    r2 = make_model("iba", "iterative_second_order", rtsolver_options=dict(n_max_stream=6, m_max=3, **opts)).run(sensor, sps)
    a, b = np.asarray(r1.data.values), np.asarray(r2.data.values)
    axis = list(r2.data.dims).index("contribution")
    assert np.array_equal(np.take(a, range(1, 5), axis), np.take(b, range(1, 5), axis))


def test_the_c_abi_refuses_emmodels_evaluated_by_the_caller(ctx):
    """A batch packed by first order with an emmodel evaluated on the host (SMRT_EM_HOST kinds), given stream and mode
    counts this solver accepts: the second-order upload refuses it before anything is uploaded."""
    from smrt_amd.core.error import SMRTError
    from smrt_amd.rtsolver.iterative_first_order import IterativeFirstOrder

    case = next(c for c in CASES if c["name"] == "iba_exp_L3_flat")
    batch = T.pack_with(case, IterativeFirstOrder(), T.Forwarding)
    assert (batch.layer_kind & 15 == _native.EM_CODES["host"]).all()
    batch.struct.n_max_stream, batch.struct.m_max = 8, 3
    with pytest.raises(SMRTError, match="smrt_second_order_run_pairs failed.*SMRT_EM_HOST"):
        ctx.second_order_run(batch)
    with pytest.raises(SMRTError, match="smrt_second_order_upload_pairs failed.*SMRT_EM_HOST"):
        ctx.second_order_upload(batch)


def test_documentation_example_runs():
    sps = [build_snowpack(c, T.api()) for c in CASES if c["name"] in ("iba_exp_L3_go", "iba_exp_L3_flat")]
    m = make_model("iba", "iterative_second_order", rtsolver_options={"return_contributions": True})
    res = m.run(sensor_list.active(13e9, [20, 35, 50]), sps)
    hv = np.asarray(res.sigmaHV_dB(contribution="total"))
    assert np.isfinite(hv).all() and np.isfinite(np.asarray(res.sigmaVV_dB(contribution="order2_intralayer_scattering"))).all()
