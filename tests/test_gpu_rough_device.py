"""Rough boundaries evaluated on the GPU (smrt_amd/csrc/rough_boundary_kernel.hpp): the builder's read-back entry point against
the NumPy evaluators on the cases and at the bar of tests/test_rough_device_cpu.py; end to end through make_interface /
make_soil -> Model.run against the reference's results in the fixtures (1e-6 K, 1e-8 relative for sigma VV / HH), with no rough
matrix uploaded; and the device route against the host route of the same objects on random snowpacks (2e-6 K / 2e-8 relative:
each route is held to half of that against the reference).  Every test prints its largest difference."""
import warnings

import numpy as np
import pytest

from conftest import ROUGH_INTERFACE_MODELS, ROUGH_OPTION_CASES, ROUGH_SUBSTRATE_MODELS, load_golden, snowpack_dict
from test_hostemu_kernel import check_rough_option_case
from test_rough_device_cpu import CASES, HostRoute, compare, pack_both, resolve

from smrt_amd import make_interface, make_model, make_snowpack, make_soil, sensor_list
from smrt_amd.rtsolver.dort import get_context

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    c = get_context()
    yield c
    c.__dict__.pop("rough_on_device", None)   # (pack_both switches the capability on the instance)


@pytest.mark.parametrize("name", sorted(CASES))
def test_builder_against_the_numpy_evaluators(ctx, name):
    layers, where, model, mode, options, frequency = resolve(CASES[name])
    device, host = pack_both(ctx, layers, where, model, mode, frequency, **options)
    compare(ctx.rough_matrices(device), host, "GPU builder " + name)
    info = ctx.rough_info()
    assert info["built_bytes"] > 0 and info["host_matrix_bytes"] == 0


def run_fixture(d, pack):
    f = float(d["frequency"][0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if str(d["mode"]) == "A":
            opts = dict(n_max_stream=int(d["opt_n_max_stream"]), m_max=int(d["opt_m_max"]))
            res = make_model("iba", "dort", rtsolver_options=opts).run(sensor_list.active(f, list(d["theta_inc_deg"])), pack)
            fac = 4 * np.pi * np.cos(np.deg2rad(d["theta_inc_deg"]))
            got = np.array([np.ravel(res.sigmaVV()), np.ravel(res.sigmaHH())])
            ref = np.array([fac * d["result"][0, 0, 0], fac * d["result"][0, 1, 1]])
            err = np.abs(got / ref - 1.0).max()
            return err, 1e-8, "relative"
        opts = dict(n_max_stream=int(d["opt_n_max_stream"]))
        res = make_model("iba", "dort", rtsolver_options=opts).run(sensor_list.passive(f, list(d["theta_deg"])), pack)
        got = np.array([np.ravel(res.TbV()), np.ravel(res.TbH())])
        return np.abs(got - np.array([d["result"][0, 0], d["result"][0, 1]])).max(), 1e-6, "K"


@pytest.mark.parametrize("route", ["device", "host"])
@pytest.mark.parametrize("name", sorted(ROUGH_INTERFACE_MODELS) + sorted(ROUGH_SUBSTRATE_MODELS))
def test_end_to_end_against_the_reference(ctx, name, route):
    """Both routes against the reference at the package's contract: the dense host route (the objects behind HostRoute) stays
    the fallback of every foreign object, and keeps its own anchor."""
    wrap = HostRoute if route == "host" else (lambda o: o)
    d = load_golden(name)
    sp = snowpack_dict(d)
    itf, substrate = ["flat"] * len(sp["thickness"]), None
    if name in ROUGH_INTERFACE_MODELS:
        model, kw = ROUGH_INTERFACE_MODELS[name]
        itf[int(d["rough_interface"][0])] = wrap(make_interface(model, **kw))
    else:
        model, kw = ROUGH_SUBSTRATE_MODELS[name]
        substrate = wrap(make_soil(model, complex(8.0, 1.0), 268.0, **kw))
    err, bar, unit = run_fixture(d, make_snowpack(sp["thickness"], "exponential", density=sp["density"], temperature=sp["temperature"],
                                                  corr_length=sp["corr_length"], interface=itf, substrate=substrate))
    info = ctx.rough_info()
    print(f"{name} on the {route} route: largest difference to the reference {err:.3e} {unit}; builder {info['builder_ms']:.3f} ms")
    assert err < bar
    if route == "host":
        assert info["built_bytes"] == 0, "nothing was built on the device"
    else:
        assert info["built_bytes"] > 0 and info["host_matrix_bytes"] == 0, "no rough matrix was uploaded"


@pytest.mark.parametrize("name", ["rough_prune_iem_L4_n10_passive", "rough_prune_go_L4_n10_active"])
def test_prune_deep_snowpack_on_the_device_route(ctx, name):
    check_rough_option_case(name, ROUGH_OPTION_CASES[name])
    info = ctx.rough_info()
    assert info["built_bytes"] > 0 and info["host_matrix_bytes"] == 0, "no rough matrix was uploaded"


@pytest.mark.parametrize("mode", ["P", "A"])
def test_device_route_against_the_host_route_on_random_snowpacks(ctx, mode):
    """32 snowpacks of two or three layers, one of the three models at the surface, an inner interface or the substrate, inside
    the validity ranges of the models (no case is left out); passive, and active with m_max 1."""
    rng = np.random.default_rng(2024)
    specs = []
    for _ in range(32):
        n = int(rng.integers(2, 4))
        model = ["geometrical_optics", "geometrical_optics_backscatter", "iem_fung92"][int(rng.integers(0, 3))]
        # (iem_fung92 holds for k s < 3 and k s . k l < sqrt(eps_r): at most 0.65 against 0.8 here at 36.5 GHz)
        kw = dict(roughness_rms=rng.uniform(1.5e-4, 2e-4), corr_length=rng.uniform(2e-3, 3e-3)) \
            if model == "iem_fung92" else dict(mean_square_slope=rng.uniform(0.02, 0.08), shadow_correction=bool(rng.integers(0, 2)))
        specs.append(dict(thickness=list(rng.uniform(0.1, 0.6, n - 1)) + [rng.uniform(2.0, 5.0)], density=list(rng.uniform(180, 420, n)),
                          temperature=list(rng.uniform(245, 268, n)), corr_length=list(rng.uniform(5e-5, 3e-4, n)),
                          where=int(rng.integers(0, n + 1)), model=model, kw=kw, eps=complex(rng.uniform(4, 10), rng.uniform(0.1, 1.0))))

    def packs(wrap):
        out = []
        for s in specs:
            n = len(s["thickness"])
            itf, substrate = ["flat"] * n, None
            if s["where"] == n:
                substrate = wrap(make_soil(s["model"], s["eps"], 268.0, **s["kw"]))
            else:
                itf[s["where"]] = wrap(make_interface(s["model"], **s["kw"]))
            out.append(make_snowpack(s["thickness"], "exponential", density=s["density"], temperature=s["temperature"],
                                     corr_length=s["corr_length"], interface=itf, substrate=substrate))
        return out

    freqs = [13.4e9, 36.5e9]
    if mode == "P":
        model, sensor = make_model("iba", "dort", rtsolver_options=dict(n_max_stream=8)), sensor_list.passive(freqs, [30.0, 50.0])
    else:
        model, sensor = make_model("iba", "dort", rtsolver_options=dict(n_max_stream=8, m_max=1)), sensor_list.active(freqs, [30.0, 50.0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        device = model.run(sensor, packs(lambda o: o))
        built = ctx.rough_info()
        host = model.run(sensor, packs(HostRoute))
        uploaded = ctx.rough_info()
    assert built["built_bytes"] > 0 and built["host_matrix_bytes"] == 0 and uploaded["host_matrix_bytes"] > 0 and uploaded["built_bytes"] == 0
    if mode == "P":
        a, b = np.asarray(device.data.values), np.asarray(host.data.values)
        err, bar, unit = np.abs(a - b).max(), 2e-6, "K"
    else:
        a = np.array([np.asarray(device.sigmaVV()), np.asarray(device.sigmaHH())])
        b = np.array([np.asarray(host.sigmaVV()), np.asarray(host.sigmaHH())])
        err, bar, unit = np.abs(a / b - 1.0).max(), 2e-8, "relative"
    print(f"32 random snowpacks, mode {mode}, device route against host route: largest difference {err:.3e} {unit}")
    assert np.isfinite(a).all() and err < bar


def test_nan_boundary_outside_validity_as_on_the_host_route(ctx):
    """warning_handling "nan" on an iem_fung92 surface that is inside its range at 5 GHz and outside at 89 GHz (k s = 0.5 and
    9): the device route gives NaN where the host route of the same object does, and its numbers elsewhere."""
    def pack(wrap):
        iem = make_interface("iem_fung92", roughness_rms=0.005, corr_length=0.001, warning_handling="nan")
        return make_snowpack([0.3, 10.0], "exponential", density=[250, 350], temperature=[260, 265], corr_length=[1e-4, 2e-4],
                             interface=[wrap(iem), "flat"])

    from smrt_amd.core.error import SMRTError

    sensor = sensor_list.passive([5e9, 89e9], [30.0, 50.0])
    model = make_model("iba", "dort", rtsolver_options=dict(n_max_stream=8, error_handling="nan"))
    strict = make_model("iba", "dort", rtsolver_options=dict(n_max_stream=8))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        device = np.asarray(model.run(sensor, pack(lambda o: o)).data.values)
        host = np.asarray(model.run(sensor, pack(HostRoute)).data.values)
        for wrap in (lambda o: o, HostRoute):     # error_handling "exception": the same error on both routes
            with pytest.raises(SMRTError, match="singular"):
                strict.run(sensor, pack(wrap))
    assert np.array_equal(np.isnan(device), np.isnan(host))
    assert np.isnan(device).any() and np.isfinite(device).any()
    err = np.nanmax(np.abs(device - host))
    print(f"iem_fung92 under 'nan': {int(np.isnan(device).sum())} of {device.size} values NaN on both routes; elsewhere {err:.3e} K apart")
    assert err < 2e-6
