"""Rough boundaries evaluated on the GPU (smrt_amd/csrc/rough_boundary_kernel.hpp): the builder's read-back entry point against
the NumPy evaluators on the cases and at the bar of tests/test_rough_device_cpu.py; end to end through make_interface /
make_soil -> Model.run against the reference's results in the fixtures (1e-6 K, 1e-8 relative for sigma VV / HH), with no rough
matrix uploaded; and the device route against the host route of the same objects on random snowpacks (2e-6 K / 2e-8 relative:
each route is held to half of that against the reference).  Whole batches (BATCH_CASES of the CPU file) go through the same
read-back at the same bar and an exact structure; pair windows, pair lists, launches split by the workspace budget and a refused
snowpack among good ones go through the solve, against the host route at the bars between the routes; a large upload, a small
one and the large one again are compared by bytes.  Every test prints its largest difference."""
import warnings

import numpy as np
import pytest

from conftest import ROUGH_INTERFACE_MODELS, ROUGH_OPTION_CASES, ROUGH_SUBSTRATE_MODELS, load_golden, snowpack_dict
from test_hostemu_kernel import check_rough_option_case
from test_rough_device_cpu import (BATCH_CASES, CASES, MIXED_RAGGED_OF, REFUSED_MIDDLE, REFUSED_ROUGH, TWO_FREQUENCIES, HostRoute,
                                   SharedBatches, batch_snowpack, check_refused_rough, check_structure, compare, pack_batch, pack_both,
                                   pack_route, refused_options, resolve)

from smrt_amd import make_interface, make_model, make_snowpack, make_soil, sensor_list
from smrt_amd._native import rough_matrix_bytes
from smrt_amd.rtsolver.dort import DORT, get_context

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    c = get_context()
    yield c
    c.__dict__.pop("rough_on_device", None)   # (pack_both switches the capability on the instance)


@pytest.fixture(scope="module")
def shared():
    """The batch cases as packed through the GPU context by the tests of this module (the CPU file keeps its own)."""
    return SharedBatches()


@pytest.mark.parametrize("name", sorted(CASES))
def test_builder_against_the_numpy_evaluators(ctx, name):
    layers, where, model, mode, options, frequency = resolve(CASES[name])
    device, host = pack_both(ctx, layers, where, model, mode, frequency, **options)
    compare(ctx.rough_matrices(device), host, "GPU builder " + name)
    info = ctx.rough_info()
    assert info["built_bytes"] > 0 and info["host_matrix_bytes"] == 0


@pytest.mark.parametrize("name", sorted(BATCH_CASES))
def test_builder_on_whole_batches_against_the_numpy_evaluators(ctx, shared, name):
    """Several snowpacks x frequencies, ragged layer counts, up to three boundaries per snowpack and the three kinds in one
    launch: the matrices at the bar of the single cases, the slot table and every empty region exactly."""
    device, host = shared.case(ctx, name)
    layer_eps = shared.layer_eps(ctx, name)      # (a launch of its own: before the build, whose rough_info is read below)
    built = ctx.rough_matrices(device)
    check_structure(built, device, host, layer_eps, "GPU builder " + name)
    compare(built, host, "GPU builder " + name)
    info = ctx.rough_info()
    assert info["built_bytes"] > 0 and info["host_matrix_bytes"] == 0


def route_difference(mode, got, expected):
    """(largest difference, bar, unit) between the two routes: kelvin in passive mode, relative on sigma VV and HH in active."""
    if mode == "P":
        return float(np.abs(got - expected).max()), 2e-6, "K"
    a = np.array([got[:, 0, 0], got[:, 1, 1]])
    b = np.array([expected[:, 0, 0], expected[:, 1, 1]])
    return float(np.abs(a / b - 1.0).max()), 2e-8, "relative"


@pytest.mark.parametrize("mode", ["P", "A"])
def test_pair_window_and_pair_list_solve_as_the_host_route(ctx, shared, mode):
    """The builder's workspace is indexed by the position in the upload, its outputs by the global pair: a window across the
    frequency boundary and an unordered list with gaps, solved on the device route, against the same pairs of the host
    route run whole.  (A wrong pair index is kelvins, not 1e-6.)"""
    device, host = shared.case(ctx, MIXED_RAGGED_OF[mode])
    assert device.n_pairs == 8
    whole = ctx.run(host)
    assert not whole.status.any() and np.isfinite(whole.values).all()
    for what, kw, rows in (("window (3, 4)", dict(pair_begin=3, pair_count=4), [3, 4, 5, 6]), ("list [6, 1, 4, 3]", dict(pairs=[6, 1, 4, 3]), [6, 1, 4, 3])):
        part = ctx.run(device, **kw)
        info = ctx.rough_info()
        assert info["built_bytes"] > 0 and info["host_matrix_bytes"] == 0
        assert part.status.tolist() == [0] * 4, what
        err, bar, unit = route_difference(mode, part.values, whole.values[rows])
        print(f"mixed_ragged, mode {mode}, {what}: device route against the same pairs of the host route {err:.3e} {unit}")
        assert np.isfinite(part.values).all() and err < bar, what


def results_of(result, mode):
    if mode == "P":
        return np.asarray(result.data.values)
    return np.array([np.asarray(result.sigmaVV()), np.asarray(result.sigmaHH())])


def test_a_group_beyond_the_workspace_budget_is_split_into_launches_on_the_device(ctx):
    """Six snowpacks with a geometrical_optics surface at two frequencies: whole, then with the budget of one snowpack's
    matrices -- more launches, the same results, both at the bar between the routes."""
    def packs(wrap):
        return [make_snowpack([0.2 + 0.1 * k, 10.0], "exponential", density=[200.0 + 30.0 * k, 350.0 + 10.0 * k], temperature=[260, 265],
                              corr_length=[1e-4, 2e-4], interface=[wrap(make_interface("geometrical_optics", mean_square_slope=0.04)), "flat"])
                for k in range(6)]

    solver = DORT(n_max_stream=8)
    model, sensor = make_model("iba", solver), sensor_list.passive([19e9, 37e9], 40.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        host = results_of(model.run(sensor, packs(HostRoute)), "P")
        whole, whole_launches = results_of(model.run(sensor, packs(lambda o: o)), "P"), solver.launches
        assert ctx.rough_info()["built_bytes"] > 0
        # one snowpack, two frequencies (on the instance, where DORT looks first: the class has a read-only property)
        ctx.__dict__["rough_workspace_budget"] = rough_matrix_bytes(2, 1, False, 8, 1)
        try:
            cut, cut_launches = results_of(model.run(sensor, packs(lambda o: o)), "P"), solver.launches
        finally:
            ctx.__dict__.pop("rough_workspace_budget", None)
    assert whole_launches == 1 and cut_launches == 6
    errs = [float(np.abs(a - host).max()) for a in (whole, cut)]
    print(f"six snowpacks x two frequencies against the host route: one launch {errs[0]:.3e} K, {cut_launches} launches {errs[1]:.3e} K; "
          f"between the two {float(np.abs(whole - cut).max()):.3e} K")
    assert whole.shape == cut.shape == host.shape and np.isfinite(host).all() and max(errs) < 2e-6


def test_a_smaller_upload_after_a_larger_one_reuses_the_buffers(ctx, shared):
    """The context's buffers are reserved once and cleared per upload: three slots with substrates, then one boundary
    without a substrate, then the first again.  By bytes: the builder has no floating-point atomics."""
    layers, where, model, mode, options, frequency = resolve(CASES["gob_inner_active"])
    small, _ = pack_both(ctx, layers, where, model, mode, frequency, **options)
    fresh = ctx.rough_matrices(small)            # before anything else of this test
    big, _ = shared.case(ctx, "mixed_ragged_active")
    first, middle, third = ctx.rough_matrices(big), ctx.rough_matrices(small), ctx.rough_matrices(big)
    assert first.slots == 3 and first.has_substrate and middle.slots == 1 and not middle.has_substrate
    differing = 0
    for key in ("slot", "itf", "itf_coh", "sub", "sub_coh"):
        for a, b in ((getattr(first, key), getattr(third, key)), (getattr(fresh, key), getattr(middle, key))):
            differing += int(np.count_nonzero(a != b))
    print(f"large, small, large on one context: {differing} elements differ from the first build / the build on the context as it was")
    for key in ("slot", "itf", "itf_coh", "sub", "sub_coh"):
        assert getattr(first, key).tobytes() == getattr(third, key).tobytes(), key
        assert getattr(fresh, key).tobytes() == getattr(middle, key).tobytes(), key
    assert first.itf.any() and first.sub.any() and middle.itf.any() and not middle.sub.any()


@pytest.mark.parametrize("mode", ["P", "A"])
def test_one_refused_snowpack_among_good_ones_as_on_the_host_route(ctx, mode):
    """Three snowpacks at two frequencies, the middle one with a layer of one stream (tests/test_rough_device_cpu.py:
    REFUSED_MIDDLE, flat itself: the host route cannot pack a rough boundary on it): both routes refuse it and nothing else,
    and the other snowpacks come out as on the host route -- through Model.run under error_handling "nan"."""
    options = refused_options(mode)
    device, host = pack_batch(ctx, REFUSED_MIDDLE, mode, TWO_FREQUENCIES, **options)
    on_device, on_host = ctx.run(device), ctx.run(host)
    assert np.array_equal(on_device.status, on_host.status)
    assert on_device.status.tolist() == [0, 5, 0, 0, 5, 0], "exactly one snowpack is refused, at both frequencies"
    model = make_model("iba", "dort", rtsolver_options=dict(options, error_handling="nan"))
    sensor = sensor_list.passive(TWO_FREQUENCIES, 40.0) if mode == "P" else sensor_list.active(TWO_FREQUENCIES, 40.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = results_of(model.run(sensor, [batch_snowpack(d) for d in REFUSED_MIDDLE]), mode)
        assert ctx.rough_info()["built_bytes"] > 0
        b = results_of(model.run(sensor, [batch_snowpack(d, HostRoute) for d in REFUSED_MIDDLE]), mode)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and 3 * int(np.isnan(a).sum()) == a.size, "one snowpack in three is NaN on both routes"
    good = ~np.isnan(a)
    err, bar, unit = (np.abs(a - b)[good].max(), 2e-6, "K") if mode == "P" else (np.abs(a / b - 1.0)[good].max(), 2e-8, "relative")
    print(f"refused middle snowpack, mode {mode}: status {on_device.status.tolist()} on both routes; the other snowpacks {err:.3e} {unit} apart")
    assert err < bar


@pytest.mark.parametrize("mode", ["P", "A"])
def test_the_builder_builds_nothing_for_a_refused_pair_with_rough_boundaries(ctx, mode):
    """Device route only (REFUSED_ROUGH): the refused snowpack carries the three kinds and a rough soil; the solve refuses
    its pairs with status 5 and the builder builds none of its boundaries."""
    device = pack_route(ctx, REFUSED_ROUGH, mode, TWO_FREQUENCIES, True, **refused_options(mode))
    built = ctx.rough_matrices(device)
    check_refused_rough(device, ctx.run(device).status, built, f"GPU builder, refused rough snowpack, mode {mode}")


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
