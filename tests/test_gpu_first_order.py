"""The iterative first-order solver on the GPU: every fixture through the C ABI and through Model.run, a random batch
against the NumPy restatement, batching (bitwise equal to single solves, one launch), error handling, the analytic
identity of a semi-infinite layer, a 10^5-item call and protocol-only objects.  Tolerance as in test_first_order_cpu.py:
1e-8 of the solve's largest co-polarised total for every element.

Worst figures of the fixtures on the MI355X: profiles/first_order_parity.txt."""
import types
import warnings

import numpy as np
import pytest

from first_order_restatement import CASES, CONTRIBUTIONS, SIGMA_RTOL, build_snowpack, first_order
from oracle import dort_oracle as O
from smrt_amd import make_model, sensor_list
from smrt_amd.inputs.make_medium import make_interface, make_snowpack, make_soil
from test_first_order_cpu import api, assert_matches_fixture, golden, pack_case, scale_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from smrt_amd.rtsolver.dort import get_context

    return get_context()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_through_the_c_abi(case, ctx):
    batch, extras = pack_case(case, ctx.first_order_run)   # (pack_case reads .layers of what this returns)
    out = ctx.first_order_run(batch, extras)
    assert out.status[0] == 0
    L = len(case["thickness"])
    assert_matches_fixture(case, out.values[0], out.layer_backscatter[0][:L + 1], out.layers[0][:L], "C ABI")
    # the split form gives the same bits
    ctx.first_order_upload(batch, extras)
    ctx.first_order_launch()
    ctx.first_order_sync()
    again = ctx.first_order_download()
    assert np.array_equal(again.values, out.values) and np.array_equal(again.layer_backscatter, out.layer_backscatter)
    ms = ctx.first_order_kernel_ms()
    assert ms[0] > 0 and ms[1] > 0


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_through_model_run(case):
    sp = build_snowpack(case, api())
    m = make_model(case["emmodel"], "iterative_first_order", rtsolver_options={"return_contributions": True})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = m.run(sensor_list.active(case["frequency"], case["theta"]), sp)
    assert res.data.dims == ("contribution", "theta_inc", "polarization_inc", "polarization")
    assert list(res.data.coords["contribution"]) == CONTRIBUTIONS
    g = golden(case)
    L = len(case["thickness"])
    assert np.abs(res.data.values - g["contributions"]).max() <= SIGMA_RTOL * scale_of(g)
    lb = res.other_data["backscatter_layer"]
    assert list(lb.coords["layer"]) == list(range(-1, L))
    scalars = np.column_stack([res.other_data["effective_permittivity"].values.real, res.other_data["effective_permittivity"].values.imag,
                               res.other_data["ks"].values, res.other_data["ka"].values])
    assert_matches_fixture(case, res.data.values[1:], lb.values, scalars, "Model.run")
    assert np.allclose(res.other_data["ks"].values, g["ks"], rtol=1e-11, atol=0) and np.allclose(res.other_data["ka"].values, g["ka"], rtol=1e-10, atol=0)
    assert np.allclose(res.optical_depth().values, (g["ks"] + g["ka"]) * np.array(case["thickness"]), rtol=1e-10)
    assert np.allclose(res.single_scattering_albedo().values, g["ks"] / (g["ks"] + g["ka"]), rtol=1e-10, atol=1e-300)
    # the accessors of ActiveResult, with and without a selection on the contribution
    theta = np.deg2rad(case["theta"])
    vv = 4 * np.pi * np.cos(theta) * g["contributions"][:, :, 0, 0]
    assert np.allclose(res.sigmaVV(contribution="total"), vv[0], rtol=1e-7)
    assert np.allclose(res.sigmaVV(contribution="order1_double_bounce"), vv[3], rtol=1e-7, atol=1e-8 * vv[0].max())
    if (vv[3] > 0).all():   # (a mechanism that is exactly absent has no dB value)
        assert np.allclose(res.sigmaVV_dB(contribution="order1_double_bounce"), 10 * np.log10(vv[3]), atol=1e-6)
    total_only = make_model(case["emmodel"], "iterative_first_order")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res0 = total_only.run(sensor_list.active(case["frequency"], case["theta"]), sp)
    assert res0.data.dims == ("theta_inc", "polarization_inc", "polarization")
    assert np.array_equal(res0.data.values, res.data.values[0])


def random_snowpacks(n, seed=11):
    rng = np.random.RandomState(seed)
    soil = lambda k: [None, make_soil("flat", complex(rng.uniform(3, 10), rng.uniform(0.1, 1.5)), 268.0),   # noqa: E731
                      api().make_reflector(specular_reflection={"V": rng.uniform(0.1, 0.9), "H": rng.uniform(0.1, 0.9)}),
                      make_soil("iem_fung92", complex(8.0, 1.0), 268.0, roughness_rms=0.004, corr_length=0.05, warning_handling="none"),
                      make_soil("geometrical_optics_backscatter", complex(6.0, 0.5), 268.0, mean_square_slope=rng.uniform(0.03, 0.1))][k]
    packs, specs = [], []
    for i in range(n):
        L = int(rng.randint(1, 8))
        spec = dict(thickness=rng.uniform(0.01, 0.6, L), density=rng.uniform(150, 450, L), temperature=rng.uniform(245, 272, L),
                    corr_length=rng.uniform(5e-5, 4e-4, L))
        sub = soil(i % 5)
        packs.append(make_snowpack(spec["thickness"], "exponential", density=spec["density"], temperature=spec["temperature"],
                                   corr_length=spec["corr_length"], substrate=sub))
        specs.append((spec, i % 5, sub))
    return packs, specs


def test_random_batch_against_the_restatement():
    """3000 snowpacks of 1..7 layers on all five kinds of substrate (none, flat, reflector, iem_fung92,
    geometrical_optics_backscatter) x 4 angles."""
    packs, specs = random_snowpacks(3000)
    theta = [15.0, 30.0, 45.0, 60.0]
    m = make_model("iba", "iterative_first_order", rtsolver_options={"return_contributions": True})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = m.run(sensor_list.active(13.4e9, theta), packs)
    assert res.data.dims[:2] == ("snowpack", "contribution")
    worst = 0.0
    for i, (spec, kind, sub) in enumerate(specs):
        sp = dict(microstructure="exponential", **spec)
        layers = O.make_layers("iba", 13.4e9, sp)
        if kind == 1:
            sub = ("flat", sub.permittivity(13.4e9))
        elif kind == 2:
            sub = ("reflector", sub.specular_reflection["V"], sub.specular_reflection["H"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref, _ = first_order(layers, spec["thickness"], 13.4e9, theta, None, sub)
        total = ref.sum(axis=0)
        scale = max(total[:, 0, 0].max(), total[:, 1, 1].max())
        err = max(np.abs(res.data.values[i, 1:] - ref).max(), np.abs(res.data.values[i, 0] - total).max()) / scale
        worst = max(worst, err)
    print(f"random batch: worst error {worst:.2e} of the largest co-polarised total")
    assert worst <= SIGMA_RTOL


def test_model_run_equals_single_solves_bitwise_in_one_launch():
    from smrt_amd.rtsolver.iterative_first_order import IterativeFirstOrder

    packs, _ = random_snowpacks(40, seed=5)
    packs = [p for k, p in enumerate(packs) if k % 5 == 1]   # one substrate kind: one homogeneous group
    sensor = sensor_list.active([5.405e9, 13.4e9, 17.25e9], [20.0, 35.0, 50.0])
    m = make_model("iba", "iterative_first_order", rtsolver_options={"return_contributions": True})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = m.run(sensor, packs)
        assert res.data.dims[:2] == ("frequency", "snowpack") and res.data.shape[:2] == (3, len(packs))
        solver = IterativeFirstOrder(return_contributions=True)
        plan = m.plan(sensor, packs)
        solver.solve_plan(m, plan)
        assert solver.launches == 1
        for fi, s in enumerate(sensor.split(["frequency"])):
            for k, sp in enumerate(packs):
                single = m.run_single_simulation((s, sp), None, None)
                assert np.array_equal(single.data.values, res.data.values[fi, k])
                assert np.array_equal(single.other_data["backscatter_layer"].values,
                                      res.other_data["backscatter_layer"].values[fi, k][:sp.nlayer + 1])


def test_error_handling_nan_leaves_the_other_snowpacks_untouched():
    from smrt_amd.core.error import SMRTError

    packs, _ = random_snowpacks(10, seed=3)
    packs = [p for k, p in enumerate(packs) if k % 5 == 0]
    bad = make_snowpack([0.3, 0.5], "exponential", density=[300.0, 350.0], temperature=[280.0, 260.0], corr_length=[2e-4, 2e-4])
    sensor = sensor_list.active(13.4e9, [30.0, 40.0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clean = make_model("iba", "iterative_first_order").run(sensor, packs)
        mixed = make_model("iba", "iterative_first_order", rtsolver_options={"error_handling": "nan"}).run(sensor, [packs[0], bad, packs[1]])
        assert np.isnan(mixed.data.values[1]).all()
        assert np.array_equal(mixed.data.values[0], clean.data.values[0]) and np.array_equal(mixed.data.values[2], clean.data.values[1])
        with pytest.raises(SMRTError):
            make_model("iba", "iterative_first_order").run(sensor, [packs[0], bad])


def test_semi_infinite_layer_under_a_transparent_interface():
    """sigmaVV 2 ke / mu = P_vv(-mu, mu) x refraction factor x 4 pi mu0 / (4 pi): one very deep layer, no reflection."""
    sp = make_snowpack([10000.0], "exponential", density=[300.0], temperature=[260.0], corr_length=[2e-4],
                       interface=[make_interface("transparent")])
    theta = np.array([20.0, 40.0])
    res = make_model("iba", "iterative_first_order").run(sensor_list.active(13e9, theta), sp)
    lay = O.make_layers("iba", 13e9, dict(thickness=[10000.0], density=[300.0], temperature=[260.0], microstructure="exponential",
                                          corr_length=[2e-4]))[0]
    mu0 = np.cos(np.deg2rad(theta))
    eps = complex(lay.eps_eff)
    mu = np.sqrt(eps - (1 - mu0 ** 2)).real / np.sqrt(eps).real
    refraction = (1.0 / eps.real) * (mu0 / mu)
    for t in range(2):
        p_vv = lay.phase(-mu[t], mu[t], np.pi, 2)[0, 0, 0, 0, 0] / (4 * np.pi)
        expected = p_vv * refraction[t] / (2 * (lay.ks + lay.ka))
        assert abs(res.data.values[t, 0, 0] - expected) <= 1e-8 * expected
        assert abs(res.sigmaVV(theta_inc=theta[t]) - 4 * np.pi * mu0[t] * expected) <= 1e-8 * 4 * np.pi * expected


def test_one_call_with_a_hundred_thousand_items(ctx):
    from smrt_amd._native import PackedBatch

    rng = np.random.RandomState(2)
    S, L = 12800, 6
    theta = np.deg2rad(np.linspace(20, 55, 8))
    batch = PackedBatch(np.full(S, L), rng.uniform(0.05, 0.5, (S, L)), rng.uniform(0.15, 0.45, (S, L)), rng.uniform(245, 272, (S, L)),
                        rng.uniform(5e-5, 4e-4, (S, L)), None, [13.4e9], theta, mode="A",
                        substrate=("flat", np.full((1, S), 6.0), np.full((1, S), 0.5), np.full(S, 268.0)))
    assert batch.n_pairs * len(theta) >= 100000
    out = ctx.first_order_run(batch)
    assert not out.status.any() and np.isfinite(out.values).all() and (out.values[:, 1, :, 0, 0] > 0).all()
    pick = [0, 777, S - 1]
    few = ctx.first_order_run(batch, pairs=pick)
    assert np.array_equal(few.values, out.values[pick]) and np.array_equal(few.layer_backscatter, out.layer_backscatter[pick])


def test_protocol_only_objects():
    """Emmodel, interface and substrate objects that only speak the reference's protocol (no smrt_amd base class)."""
    from smrt_amd.rtsolver.iterative_first_order import IterativeFirstOrder

    case = next(c for c in CASES if c["name"] == "iba_exp_L3_flat")

    class Emmodel:
        def __init__(self, frequency, layer):
            self._em = O.IBALayer(frequency, layer.frac_volume, layer.temperature, "exponential", corr_length=layer.microstructure.corr_length)

        def effective_permittivity(self):
            return self._em.eps_eff

        def ks(self, mu, npol=2):
            return self._em.ks

        def ka(self, mu, npol=2):
            return self._em.ka

        def phase(self, mu_s, mu_i, dphi, npol=2):
            return types.SimpleNamespace(values=self._em.phase(mu_s, mu_i, dphi, npol))

    class FresnelInterface:   # Flat, restated as an object of the caller
        def specular_reflection_matrix(self, frequency, eps_1, eps_2, mu1, npol):
            return O.flat_reflection(eps_1, eps_2, np.atleast_1d(mu1), npol)

        def coherent_transmission_matrix(self, frequency, eps_1, eps_2, mu1, npol):
            return O.flat_transmission(eps_1, eps_2, np.atleast_1d(mu1), npol)

    class Soil:
        def specular_reflection_matrix(self, frequency, eps_1, mu1, npol):
            return O.flat_reflection(eps_1, complex(8.0, 1.0), np.atleast_1d(mu1), npol)

    sp = make_snowpack(case["thickness"], "exponential", density=case["density"], temperature=case["temperature"],
                       corr_length=case["corr_length"], interface=[FresnelInterface() for _ in range(3)], substrate=Soil())
    sensor = sensor_list.active(case["frequency"], case["theta"])
    res = IterativeFirstOrder(return_contributions=True).solve(sp, [Emmodel(case["frequency"], lay) for lay in sp.layers], sensor)
    assert_matches_fixture(case, res.data.values[1:], res.other_data["backscatter_layer"].values, None, "protocol objects")


def test_split_form_with_a_pair_list(ctx):
    """upload / launch / sync / download on a sparse pair list equals the one-shot call on the same list; the upload has
    finished with the caller's arrays when it returns (the pair list handed over here is a temporary)."""
    from smrt_amd._native import PackedBatch

    rng = np.random.RandomState(9)
    S, L, F = 300, 5, 2
    theta = np.deg2rad([20.0, 40.0, 60.0])
    batch = PackedBatch(rng.randint(1, L + 1, S), rng.uniform(0.05, 0.5, (S, L)), rng.uniform(0.15, 0.45, (S, L)),
                        rng.uniform(245, 272, (S, L)), rng.uniform(5e-5, 4e-4, (S, L)), None, [13.4e9, 17.25e9], theta, mode="A",
                        substrate=("flat", np.full((F, S), 6.0), np.full((F, S), 0.5), np.full(S, 268.0)))
    pick = rng.permutation(S * F)[:257]
    one_shot = ctx.first_order_run(batch, pairs=pick)
    with ctx.lock:
        ctx.first_order_upload(batch, pairs=[int(p) for p in pick])   # a list: the binding's int64 copy is the only array
        filler = [np.full(257, -1, np.int64) for _ in range(64)]      # reuse of freed host memory must not matter any more
        for _ in range(3):
            ctx.first_order_launch()
        ctx.first_order_sync()
        split = ctx.first_order_download()
    assert len(filler) == 64 and not one_shot.status.any()
    for name in ("values", "status", "layers", "layer_backscatter", "diag"):
        assert np.array_equal(getattr(split, name), getattr(one_shot, name)), name
    full = ctx.first_order_run(batch)
    assert np.array_equal(one_shot.values, full.values[pick])
    only_layers = ctx.first_order_layers(batch)
    assert np.array_equal(only_layers, full.layers)


def test_warnings_once_per_run_with_count_and_worst_value():
    """The deliberate difference from the reference: one warning per run for the albedo and one for optically shallow
    snowpacks without substrate, each with the number of simulations concerned and the worst value; none of the second kind
    under a Transparent substrate."""
    from smrt_amd.core.error import SMRTWarning
    from smrt_amd.substrate.transparent import Transparent

    def pack(thickness, corr_length, substrate=None):
        return make_snowpack([thickness], "exponential", density=[300.0], temperature=[260.0], corr_length=[corr_length], substrate=substrate)

    sensor = sensor_list.active([13.4e9, 37e9], [30.0, 40.0])
    m = make_model("iba", "iterative_first_order")
    # 37 GHz, 0.5 mm correlation length: albedo above 0.5; 0.2 m of fine snow: tau < 5 at both frequencies
    packs = [pack(0.2, 1e-4), pack(0.2, 5e-4), pack(1000.0, 5e-4), pack(1000.0, 1e-4)]
    with pytest.warns(SMRTWarning) as record:
        res = m.run(sensor, packs)
    albedo = res.single_scattering_albedo().values          # (frequency, snowpack, layer)
    tau = res.optical_depth().values.sum(axis=-1)
    n_high, n_shallow = int((albedo.max(axis=-1) > 0.5).sum()), int((tau < 5).sum())
    assert n_high >= 2 and n_shallow >= 2                   # the inputs do exercise both
    messages = [str(w.message) for w in record if issubclass(w.category, SMRTWarning)]
    high = [msg for msg in messages if "albedo" in msg]
    shallow = [msg for msg in messages if "optically shallow" in msg]
    assert len(high) == 1 and len(shallow) == 1 and len(messages) == 2
    assert f"in {n_high} simulation(s)" in high[0] and f"{albedo.max():.2f}" in high[0]
    assert f"{n_shallow} snowpack(s)" in shallow[0] and f"tau={tau.min():g}" in shallow[0]
    # a Transparent substrate silences the second kind only (it is another device group: still one albedo warning)
    with pytest.warns(SMRTWarning) as record:
        m.run(sensor, [pack(0.2, 1e-4, Transparent()), pack(0.2, 5e-4, Transparent())])
    messages = [str(w.message) for w in record if issubclass(w.category, SMRTWarning)]
    assert len(messages) == 1 and "albedo" in messages[0]
    # mixed groups (with and without substrate) in one run: still one warning of each kind
    with pytest.warns(SMRTWarning) as record:
        m.run(sensor, packs + [pack(0.2, 5e-4, Transparent())])
    messages = [str(w.message) for w in record if issubclass(w.category, SMRTWarning)]
    assert sorted("albedo" in msg for msg in messages) == [False, True]
    # nothing to warn about: no warning
    with warnings.catch_warnings():
        warnings.simplefilter("error", SMRTWarning)
        m.run(sensor_list.active(5.405e9, [30.0]), [pack(1000.0, 1e-4)])
