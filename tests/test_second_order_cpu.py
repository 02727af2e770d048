"""The iterative second-order solver without a GPU: plugin resolution and options, the refusals, the ctypes struct against
the library's self-description, the closed-form factors at coincident cosines, the NumPy restatement against every fixture,
and the DEVICE arithmetic (smrt_amd/csrc/second_order_kernel.hpp) compiled with g++ against every fixture and against the
restatement on a random batch.

Tolerance: every contribution, every backscatter_layer entry and the total within SIGMA_RTOL = 1e-8 of the solve's largest
co-polarised total (the project's bar for sigma0), against the fixtures and against the restatement alike."""
import ctypes as C
import functools
import os
import re
import types

import numpy as np
import pytest

import second_order_restatement as R
from host_build import host_library
from second_order_restatement import CASES, CONTRIBUTIONS, SIGMA_RTOL, build_snowpack, options_of, solve_case
from smrt_amd import _native, make_model, sensor_list
from smrt_amd.core.error import SMRTError
from smrt_amd.inputs.make_medium import make_interface, make_snowpack, make_soil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
IDS = [c["name"] for c in CASES]


def api():
    from smrt_amd.substrate.reflector import make_reflector
    from smrt_amd.substrate.transparent import Transparent

    return types.SimpleNamespace(make_snowpack=make_snowpack, make_interface=make_interface, make_soil=make_soil,
                                 make_reflector=make_reflector, transparent_substrate=Transparent)


def golden(case):
    return np.load(os.path.join(GOLDEN, "second_order_" + case["name"] + ".npz"))


def scale_of(contributions):
    return max(contributions[0][:, 0, 0].max(), contributions[0][:, 1, 1].max())


def assert_close(name, theta_deg, contributions7, layer_backscatter, ref8, ref_layer, what=""):
    """contributions7 [7, n, 2, 2], layer_backscatter [L + 1, n, 2, 2] against ref8 [8, n, 2, 2] (total first) and ref_layer.
    Returns the worst error relative to the largest co-polarised total."""
    scale = scale_of(ref8)
    err = max(np.abs(contributions7 - ref8[1:]).max(), np.abs(contributions7.sum(axis=0) - ref8[0]).max()) / scale
    # backscatter_layer is a sigma0 (4 pi mu x intensity): measured against the total on that same footing
    err_layer = np.abs(layer_backscatter - ref_layer).max() / (4 * np.pi * np.cos(np.deg2rad(theta_deg)).min() * scale)
    print(f"{what} {name}: contributions {err:.2e}, backscatter_layer {err_layer:.2e} (of the largest co-polarised total)")
    assert err <= SIGMA_RTOL and err_layer <= SIGMA_RTOL, (name, err, err_layer)
    return max(err, err_layer)


# ---- plugin, options, refusals -----------------------------------------------------------------------------------------
def test_plugin_resolution_options_and_labels():
    from smrt_amd.core.plugin import import_class
    from smrt_amd.rtsolver.iterative_first_order import IterativeFirstOrder
    from smrt_amd.rtsolver.iterative_second_order import CONTRIBUTIONS as LABELS, IterativeSecondOrder

    assert import_class("rtsolver", "iterative_second_order") is IterativeSecondOrder and issubclass(IterativeSecondOrder, IterativeFirstOrder)
    m = make_model("iba", "iterative_second_order", rtsolver_options={"return_contributions": True, "compute_scattering_interlayer": True})
    solver = m.make_rtsolver_instance()
    assert isinstance(solver, IterativeSecondOrder) and solver.return_contributions and solver.compute_scattering_interlayer
    d = IterativeSecondOrder()
    assert (d.n_max_stream, d.m_max, d.stream_mode, d.compute_scattering_interlayer, d.error_handling) == (32, 5, "most_refringent", False, "exception")
    assert LABELS == CONTRIBUTIONS and LABELS == [
        "total", "order0_backscatter", "order1_direct_backscatter", "order1_double_bounce", "order1_reflected_backscatter",
        "order2_intralayer_scattering", "order2_rough_layer_scattering", "order2_interlayer_scattering"]
    assert IterativeSecondOrder._broadcast_capability == {"theta_inc", "polarization_inc", "theta", "polarization"}
    for bad in (dict(stream_mode="uniform_air"), dict(stream_mode="air"), dict(m_max=0), dict(m_max=9), dict(n_max_stream=1),
                dict(error_handling="ignore")):
        with pytest.raises(SMRTError):
            IterativeSecondOrder(**bad)


def test_refusals():
    from smrt_amd.atmosphere.simple_isotropic_atmosphere import SimpleIsotropicAtmosphere
    from smrt_amd.rtsolver.iterative_second_order import IterativeSecondOrder

    sp = make_snowpack([1.0], "exponential", density=[300.0], temperature=[260.0], corr_length=[2e-4])
    m = make_model("iba", "iterative_second_order")
    with pytest.raises(SMRTError, match="the iterative_second_order solver is only suitable for active"):
        m.run(sensor_list.passive(37e9, 55), sp)
    with pytest.raises(SMRTError, match="the iterative_second_order solver is only suitable for active"):
        IterativeSecondOrder().solve(sp, [None], sensor_list.passive(37e9, 55))
    atmosphere = SimpleIsotropicAtmosphere(tb_down=20.0, tb_up=18.0, transmittance=0.9)
    with pytest.raises(SMRTError, match="the iterative_second_order solver can not handle atmosphere"):
        IterativeSecondOrder().solve(sp, [None], sensor_list.active(13e9, 30), atmosphere=atmosphere)
    with pytest.raises(SMRTError, match="the iterative_second_order solver can not handle atmosphere"):
        m.run(sensor_list.active(13e9, 30), atmosphere + sp)
    rough = make_snowpack([0.3, 0.5], "exponential", density=[300.0, 350.0], temperature=[260.0, 262.0], corr_length=[2e-4, 3e-4],
                          interface=[make_interface("flat"), make_interface("iem_fung92", roughness_rms=0.002, corr_length=0.05)])
    with pytest.raises(SMRTError, match="interface 1 .*IEM"):
        m.run(sensor_list.active(13e9, 30), rough)


class Forwarding:
    """An emmodel outside the IBA and Rayleigh families -- nothing the device could know (its numbers are the CPU oracle's
    IBA) -- that counts how often it is asked for a number."""

    asked = 0

    def __init__(self, sensor, layer):
        from oracle import dort_oracle as O

        self._em = O.IBALayer(float(sensor.frequency), layer.frac_volume, layer.temperature, "exponential",
                              corr_length=layer.microstructure.corr_length)

    def _ask(self, value):
        Forwarding.asked += 1
        return value

    def effective_permittivity(self):
        return self._ask(self._em.eps_eff)

    def ks(self, mu, npol=2):
        return self._ask(self._em.ks)

    def ka(self, mu, npol=2):
        return self._ask(self._em.ka)

    def phase(self, mu_s, mu_i, dphi, npol=2):
        return self._ask(self._em.phase(mu_s, mu_i, dphi, npol))


def pack_with(case, solver, emmodel):
    from smrt_amd.core.model import SimulationPlan

    sp = build_snowpack(case, api())
    sensor = sensor_list.active(case["frequency"], case["theta"])
    names = solver.emmodel_names(make_model(emmodel, "iterative_second_order"), SimulationPlan([sensor], [sp], np.zeros(1, int), np.zeros(1, int)))
    return solver._packer()._pack(sensor, [sp], np.array([float(case["frequency"])]), names, {})


def test_host_evaluated_emmodels_are_refused_before_they_are_evaluated():
    from smrt_amd.rtsolver.iterative_first_order import IterativeFirstOrder
    from smrt_amd.rtsolver.iterative_second_order import IterativeSecondOrder

    case = next(c for c in CASES if c["name"] == "iba_exp_L3_flat")
    Forwarding.asked = 0
    with pytest.raises(SMRTError, match="iterative_second_order solver cannot use emmodels evaluated on the host"):
        pack_with(case, IterativeSecondOrder(n_max_stream=8, m_max=3), Forwarding)
    assert Forwarding.asked == 0
    # first order's own packing takes the same emmodel (and evaluates it)
    batch = pack_with(case, IterativeFirstOrder(), Forwarding)
    assert Forwarding.asked > 0 and (batch.layer_kind & 15 == _native.EM_CODES["host"]).all()


def test_a_stream_at_the_edge_of_total_reflection_is_refused_on_the_host():
    """The host restates the device's stream selection for the substrate rows: where `relsin < 1` could fall either way the
    two stream counts could differ, so the host refuses."""
    from scipy.special import roots_legendre
    from smrt_amd.rtsolver.iterative_second_order import IterativeSecondOrder

    node = roots_legendre(16)[0][-3]
    star = 1.9 + 1e-4j
    sets = IterativeSecondOrder.stream_sets(8, [1.5 + 1e-4j, star])
    assert len(sets[1][0]) == 8 and 2 <= len(sets[0][0]) < 8 and np.all(np.diff(sets[0][0]) > 0)
    with pytest.raises(SMRTError, match="totally reflected"):
        IterativeSecondOrder.stream_sets(8, [star * (1.0 - node ** 2), star])


def test_extras_struct_matches_the_library():
    lib = _native.load_library()
    mine, theirs = _native.second_order_extras_layout(), _native.second_order_abi_layout(lib)
    assert mine == theirs and mine[0] == C.sizeof(_native.SecondOrderExtras) and len(mine) == 1 + len(_native.SecondOrderExtras._fields_)
    header = open(os.path.join(ROOT, "include", "smrt_dort.h")).read()
    body = header[header.index("typedef struct smrt_second_order_extras {"):header.index("} smrt_second_order_extras;")]
    declared = [line.split(";")[0].split()[-1].lstrip("*") for line in body.splitlines()[1:] if ";" in line]
    assert declared == [name for name, _ in _native.SecondOrderExtras._fields_]
    for name in ("out_stride", "run_pairs", "upload_pairs", "launch", "sync", "download", "kernel_ms", "abi"):
        assert "smrt_second_order_" + name in _native.EXPORTED_SYMBOLS and hasattr(lib, "smrt_second_order_" + name)
    # the first-order struct is untouched
    assert _native.first_order_extras_layout() == _native.first_order_abi_layout(lib) == [32, 0, 4, 8, 16, 24]


# ---- the restatement against the reference's fixtures --------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated():
    """Every case solved once by the restatement: name -> (contributions7, backscatter_layer, oracle layers)."""
    out = {}
    for case in CASES:
        (c, pl), layers = solve_case(case, build_snowpack(case, api()))
        out[case["name"]] = (c, pl, layers)
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_matches_the_reference(case, restated):
    c, pl, layers = restated[case["name"]]
    g = golden(case)
    assert_close(case["name"], case["theta"], c, pl, g["contributions"], g["backscatter_layer"], "restatement")
    eps = np.array([complex(lay.eps_eff) for lay in layers])
    assert np.abs(eps - g["eps"]).max() <= 1e-12 * np.abs(g["eps"]).max()


def test_fixtures_pin_the_mechanisms_and_the_findings():
    """Each order-2 mechanism exceeds 1 % of the largest co-polarised total somewhere, HV of the total is non-zero wherever
    a layer scatters, and an interlayer value is negative."""
    share, lowest = np.zeros(3), 0.0
    for case in CASES:
        c = golden(case)["contributions"]
        share = np.maximum(share, [max(c[5 + k][:, 0, 0].max(), c[5 + k][:, 1, 1].max()) / scale_of(c) for k in range(3)])
        lowest = min(lowest, c[7].min())
        assert np.all(c[0][:, 0, 1] != 0.0) and np.all(c[0][:, 1, 0] != 0.0)
    assert np.all(share > 0.01) and lowest < 0.0, (share, lowest)


# ---- the closed-form factors at coincident cosines -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_lib():
    """The device source (second_order_kernel.hpp and what it includes) compiled with g++: tests/hostemu/second_order_host.cpp."""
    lib = host_library("libsmrt_second_order_host.so", "second_order_host.cpp")
    P = C.POINTER
    lib.smrt_second_order_host_run.argtypes = [P(_native.SmrtBatch), P(_native.SecondOrderExtras), C.c_int32, P(C.c_double), P(C.c_int32),
                                               P(C.c_double), P(C.c_double), P(C.c_double)]
    lib.smrt_second_order_host_run.restype = C.c_int32
    lib.smrt_second_order_host_coef.argtypes = [C.c_int32] + [C.c_double] * 7
    lib.smrt_second_order_host_coef.restype = C.c_double
    return lib


COINCIDENCE = ((0.8, 1.5, 2.0, 0.4, 0.7), (0.5, 0.6, 3.0, 2.0, 1.0), (0.95, 4.0, 0.3, 0.1, 2.5))   # mu_i, ke_n, ke_m, d_n, d_m


def test_factors_at_and_near_coincident_cosines(host_lib):
    """The DEVICE's so2_coef_A .. F (double) against the restatement evaluated in np.longdouble, at mu' == mu_i exactly --
    the branch of the analytic limit, for D the finite part -- and at the two neighbours mu_i (1 +- h), h = 1e-6, where the
    reference's difference quotients are used; then the continuity of the device's values across the three points.

    x = tau / mu is 0.42 .. 6 in the quotients of these cases, the exponents of a whole factor add up to less than 30,
    eps = 2^-52.  The bounds, each relative to `scale`, the sum of the magnitudes of the factor's terms (A and B are a sum of
    the quotient's term and a regular one of the other sign; C, E, F and D next to the pole are plain products; for D's
    finite part the bound on its terms written below):

    * at equality there is no cancelling quotient: an exponential carries (1 + |argument|) eps, under 31 eps over the
      exponents of a factor, the 30-odd other operations 1 eps each, and 1 - g^2 with g <= exp(-0.42) doubles what g
      carries.  256 eps = 5.7e-14.
    * at the neighbours a quotient (g(mu_i) - g(mu')) / (1 / mu_i - 1 / mu'), or its kin over mu_i - mu', is a difference
      x h g of two exponentials that carry (1 + x) eps each: 2 (1 + 1 / x) eps / h <= 6.8 eps / h; the denominator is a
      difference h / mu of two numbers that carry eps each (D has two such denominators): 2 to 4 eps / h; the restatement
      is handed the same doubles mu', so nothing comes from the offset itself.  16 eps / h = 3.6e-9.
    * continuity: a factor is smooth in mu' (D: once its pole terms, odd in the offset, cancel in the mean), so the MEAN of
      the two neighbours differs from the value at mu_i by |f''| (mu h)^2 / 2 + O(h^4).  A factor is exp(-T / mu') times
      rational terms of degree <= 2 in mu', with T <= tau_n + tau_m + tau_r the optical depths of all its exponentials in mu'
      (a difference quotient of exp(-tau / mu') is a mean of its derivative and no rougher): its logarithmic derivative is
      below T / mu^2 + 2 / mu and f'' / f below (T / mu^2 + 2 / mu)^2 + 2 T / mu^3 + 2 / mu^2 =: K, so
      |mean - f(mu_i)| <= K (mu h)^2 / 2 scale -- 2.1e-10 in the worst case here (mu = 0.5, T = 8.7).  On the device's
      doubles the rounding of the neighbours adds to it: asserted at K (mu h)^2 / 2 + 16 eps / h.  For D the neighbours are
      of order residue / (mu h) and their rounding scales with THAT magnitude, so the mean is held to K (mu h)^2 / 2 scale
      + 16 eps / h |D(neighbour)|.  The neighbours are doubles, so their offsets a = mu_i - lo and b = hi - mu_i differ by a
      rounding of mu_i; the pole terms residue (1 / b - 1 / a) then leave |D(neighbour)| |a - b| / a in the sum (half of it
      in the mean): added to D's bound with a and b taken exactly.
    The restatement's own longdouble rounding (2^-63, 1e-13 after the quotients) is far below all of these."""
    ld = np.longdouble
    eps, h = 2.0 ** -52, 1e-6
    at_rtol, near_rtol = 256 * eps, 16 * eps / h
    for mu, ke_n, ke_m, d_n, d_m in COINCIDENCE:
        tau_n, tau_m = ke_n * d_n, ke_m * d_m
        tau_r = tau_n + tau_m + 0.3
        args = (ke_n, ke_m, tau_n, tau_m, tau_r)
        T = tau_n + tau_m + tau_r
        curvature = ((T / mu ** 2 + 2 / mu) ** 2 + 2 * T / mu ** 3 + 2 / mu ** 2) * (mu * h) ** 2 / 2

        def device(name, x):
            return host_lib.smrt_second_order_host_coef(ord(name), mu, x, *args)

        def restated(name, x):
            m, x, kn, km, tn, tm, tr = (ld(v) for v in (mu, x) + args)
            return {"A": lambda: R.coef_A(m, x, kn, tn), "B": lambda: R.coef_B(m, x, kn, tn),
                    "C": lambda: R.coef_C(m, x, kn, km, tn, tm, tr), "D": lambda: R.coef_D(m, x, kn, km, tn, tm, tr),
                    "E": lambda: R.coef_E(m, x, kn, tn, tr), "F": lambda: R.coef_F(m, x, kn, tn, tr)}[name]()

        def scale(name, x, value):
            if name in "AB":   # the regular term, common to both, and the quotient's term
                gi = np.exp(-ld(tau_n) / ld(mu))
                regular = (gi if name == "A" else 1) * ld(mu) * (1 - gi * gi) / (2 * ld(ke_n)) / (ld(ke_n) * (ld(mu) + ld(x)))
                return float(abs(regular) + abs(value - regular))
            if name == "D" and x == mu:   # |F'' G / 2| + |F' G'| with 1 - g^2 <= 1, g^2 <= 1
                a = ld(mu)
                k = np.exp(-(2 * ld(tau_m) + 2 * ld(tau_r)) / a) / (ld(ke_n) * ld(ke_m))
                t = ld(tau_m) / a
                return float(k * (t * t / 2 + t + t * (1 + (ld(tau_n) + ld(tau_r)) / a)))
            return float(abs(value))

        lo, hi = mu * (1 - h), mu * (1 + h)   # doubles: the device and the restatement get the same
        assert lo != mu != hi
        skew = float(abs((ld(mu) - ld(lo)) - (ld(hi) - ld(mu))) / (ld(mu) - ld(lo)))
        for name in "ABCDEF":
            d_at, d_lo, d_hi = device(name, mu), device(name, lo), device(name, hi)
            r_at, r_lo, r_hi = restated(name, mu), restated(name, lo), restated(name, hi)
            assert np.isfinite([d_at, d_lo, d_hi]).all() and d_at != 0.0, name
            s_at = scale(name, mu, r_at)
            err = [abs(d_at - float(r_at)) / s_at, abs(d_lo - float(r_lo)) / scale(name, lo, r_lo), abs(d_hi - float(r_hi)) / scale(name, hi, r_hi)]
            print(f"factor {name} at mu_i = {mu}: device - longdouble restatement at equality {err[0]:.1e}, below {err[1]:.1e}, above {err[2]:.1e}")
            assert err[0] <= at_rtol and err[1] <= near_rtol and err[2] <= near_rtol, (name, mu, err)
            if name == "D":   # the pole, and the finite part between its two branches
                assert abs(d_lo) > 1e4 * abs(d_at) and np.sign(d_lo) == -np.sign(d_hi)
                assert abs((r_lo + r_hi) / 2 - r_at) <= curvature * s_at + (1e-12 + skew) * abs(r_lo)
                assert abs((d_lo + d_hi) / 2 - d_at) <= curvature * s_at + (near_rtol + skew) * abs(d_lo), (name, mu, d_at, (d_lo + d_hi) / 2)
            else:
                assert abs((r_lo + r_hi) / 2 - r_at) <= curvature * s_at
                assert abs((d_lo + d_hi) / 2 - d_at) <= (curvature + near_rtol) * s_at, (name, mu, d_at, d_lo, d_hi)
                assert abs(d_lo - d_at) <= 1e-4 * s_at and abs(d_hi - d_at) <= 1e-4 * s_at, name   # |f'| mu h, f' / f of order 10


# ---- the device arithmetic on the CPU ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_ctx(host_lib):
    """Stands where the DortContext stands in the solver: second_order_run and first_order_layers on the host build."""
    lib = host_lib

    class HostContext:
        order = 0

        def second_order_run(self, batch, extras=None, pairs=None):
            assert pairs is None
            o = _native.SecondOrderOutput(batch, batch.n_pairs)
            assert lib.smrt_second_order_host_run(C.byref(batch.struct), C.byref(extras.struct) if extras is not None else None,
                                                  self.order, *o.pointers()) == 0
            return o

        def first_order_layers(self, batch):
            return self.second_order_run(batch).layers
    return HostContext()


def run_case(case, ctx, **options):
    """A case through the solver's own packing, the host-evaluated numbers included, on `ctx`."""
    from smrt_amd.core.model import SimulationPlan
    from smrt_amd.rtsolver.iterative_second_order import IterativeSecondOrder

    sp = build_snowpack(case, api())
    model = make_model(case["emmodel"], "iterative_second_order")
    sensor = sensor_list.active(case["frequency"], case["theta"])
    solver = IterativeSecondOrder(**{**options_of(case), **options})
    packer = solver._packer()
    names = solver.emmodel_names(model, SimulationPlan([sensor], [sp], np.zeros(1, int), np.zeros(1, int)))
    freqs = np.array([float(case["frequency"])])
    batch = packer._pack(sensor, [sp], freqs, names, {})
    extras = solver._extras(ctx.first_order_layers, batch, packer, sensor, [sp], freqs)
    return solver._run_group(ctx, batch, extras, None, packer, sensor, [sp], freqs)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_arithmetic_on_the_cpu_matches_the_reference(case, host_ctx, restated):
    out = run_case(case, host_ctx)
    assert out.status[0] == 0
    L = len(case["thickness"])
    g = golden(case)
    assert_close(case["name"], case["theta"], out.values[0], out.layer_backscatter[0][:L + 1], g["contributions"], g["backscatter_layer"], "host build")
    c, pl, _ = restated[case["name"]]
    ref8 = np.concatenate([c.sum(axis=0)[None], c])
    assert_close(case["name"], case["theta"], out.values[0], out.layer_backscatter[0][:L + 1], ref8, pl, "host build vs restatement")


def test_fiber_order_does_not_matter(host_ctx):
    case = next(c for c in CASES if c["name"] == "iba_exp_L3_go_inter")
    host_ctx.order = 0
    a = run_case(case, host_ctx)
    try:
        for order in (1, 2):
            host_ctx.order = order
            b = run_case(case, host_ctx)
            assert np.array_equal(a.values, b.values) and np.array_equal(a.layer_backscatter, b.layer_backscatter)
    finally:
        host_ctx.order = 0


def random_batch(rng, layer_counts, theta_deg, n_max_stream=6, m_max=3, density=(200.0, 420.0), substrate=None):
    """Snowpacks of the given layer counts (IBA, exponential) as cases.  `density`: the range the densities are drawn from;
    `substrate`: None (a Flat soil under every snowpack) or a function of the snowpack's index that gives its soil."""
    cases = []
    for k, L in enumerate(layer_counts):
        cases.append(dict(name=f"random_{k}", emmodel="iba", frequency=13e9, theta=list(theta_deg), thickness=list(rng.uniform(0.1, 0.6, L)),
                          density=list(rng.uniform(density[0], density[1], L)), temperature=list(rng.uniform(250.0, 270.0, L)),
                          microstructure_model="exponential", corr_length=list(rng.uniform(1e-4, 4e-4, L)),
                          substrate=substrate(k) if substrate else dict(substrate_model="flat", **R.SOIL), n_max_stream=n_max_stream,
                          m_max=m_max))
    return cases


class PackedGroup:
    """Cases (one set of angles, one n_max_stream and m_max) packed once by the solver's own packer as snowpacks x
    `frequencies` (None: the frequency of the first case), global pair = frequency index x len(cases) + snowpack index;
    run() sends it through the solver's own _extras and _run_group on a context, any number of times."""

    def __init__(self, cases, frequencies=None):
        from smrt_amd.core.model import SimulationPlan
        from smrt_amd.rtsolver.iterative_second_order import IterativeSecondOrder

        self.cases = cases
        self.sps = [build_snowpack(c, api()) for c in cases]
        self.freqs = np.array([float(f) for f in (frequencies or [cases[0]["frequency"]])])
        self.sensor = sensor_list.active(float(self.freqs[0]), cases[0]["theta"])
        self.solver = IterativeSecondOrder(n_max_stream=cases[0]["n_max_stream"], m_max=cases[0]["m_max"])
        self.solver.launches = 0
        self.host_side = None
        self.packer = self.solver._packer()
        idx = np.arange(len(self.sps))
        names = self.solver.emmodel_names(make_model("iba", "iterative_second_order"),
                                          SimulationPlan([self.sensor], self.sps, np.zeros(len(self.sps), int), idx))
        self.batch = self.packer._pack(self.sensor, self.sps, self.freqs, names, {})

    def run(self, ctx, interlayer, workspace_budget=None, pairs=None):
        """What the host evaluates for the batch (first order's extras, the substrate's modes) depends on none of the
        arguments but the context: evaluated by the solver's own methods on the first run on a context, kept for the next."""
        s = self.solver
        s.compute_scattering_interlayer, s.workspace_budget = bool(interlayer), workspace_budget
        if self.host_side is None or self.host_side[0] is not ctx:
            self.host_side = (ctx, s._extras(ctx.first_order_layers, self.batch, self.packer, self.sensor, self.sps, self.freqs),
                              type(s)._substrate_modes(s, ctx, self.batch, self.sensor, self.sps, self.freqs))
            s._substrate_modes = lambda *args: self.host_side[2]
        return s._run_group(ctx, self.batch, self.host_side[1], pairs, self.packer, self.sensor, self.sps, self.freqs)


def solve_batch_on(ctx, cases, interlayer, frequencies=None):
    group = PackedGroup(cases, frequencies)
    return group.run(ctx, interlayer), group.sps


def test_device_arithmetic_on_a_random_batch_matches_the_restatement(host_ctx):
    rng = np.random.RandomState(11)
    cases = random_batch(rng, [1, 2, 3, 5, 3, 2], [20.0, 35.0, 50.0])
    for interlayer in (False, True):
        out, sps = solve_batch_on(host_ctx, cases, interlayer)
        assert not out.status.any()
        for k, (case, sp) in enumerate(zip(cases, sps)):
            (c, pl), _ = solve_case(dict(case, interlayer=interlayer), sp)
            L = len(case["thickness"])
            assert_close(case["name"], case["theta"], out.values[k], out.layer_backscatter[k][:L + 1], np.concatenate([c.sum(axis=0)[None], c]), pl,
                         "host build, interlayer" if interlayer else "host build")
            assert not out.layer_backscatter[k][L + 1:].any()


# ---- the edge shapes (tests/test_gpu_second_order_edges.py runs the same batches on the GPU) ------------------------------
def test_edge_fixtures_are_sensitive():
    """A fixture that a wrong kernel would pass proves nothing: the conditions on the inputs of the edge cases
    (second_order_restatement.EDGE_CASES), each checked on the restatement alone.  The margins are relative to the largest
    co-polarised total of the case, as SIGMA_RTOL is.

    Streams past lane 63 -- every case with more than 64 streams in a layer, evaluated again with every layer's stream set
    cut to its first 64 (a wavefront whose lanes take one trip only): an order-2 contribution must move by more than
    1000 SIGMA_RTOL = 1e-5 -- the intralayer term always, the interlayer term where two layers of the snowpack both have
    more than 64 streams (it stops at the shorter set).  Measured (intralayer / interlayer): iba_exp_L2_n65_inter, sets
    48 / 65, 1.3e-4 / 0;  iba_exp_contrast_L3_n130_inter, sets 60 / 130 / 66, 1.4e-3 / 1.3e-4.

    Top mode -- every m_max = k case with k in 4, 6, 7, 8, against the same input at m_max = k - 1: an order-2 contribution
    must move by more than 100 SIGMA_RTOL = 1e-6.  Measured (intralayer / substrate / interlayer):
    k = 4: 2.2e-2 / 6.9e-3 / 1.8e-3;  k = 6: 2.5e-4 / 5.9e-4 / 6.5e-6;  k = 7: 2.3e-5 / 2.3e-4 / 4.8e-7;
    k = 8: 2.1e-6 / 8.5e-5 / 3.2e-8.  No k is dropped; the interlayer term alone would not hold k = 7 and 8.

    The stream sets the cases are built for are asserted too: 47 / 64, 48 / 65, 60 / 130 / 66 and 7 / 16 / 8."""
    from smrt_amd.rtsolver.iterative_second_order import IterativeSecondOrder

    by_name = {c["name"]: c for c in R.EDGE_CASES}
    counts = {}
    for case in R.EDGE_CASES:
        sp = build_snowpack(case, api())
        (full, _), layers = solve_case(case, sp)
        scale = scale_of(np.concatenate([full.sum(axis=0)[None], full]))
        sets = IterativeSecondOrder.stream_sets(case["n_max_stream"], [complex(lay.eps_eff) for lay in layers])
        counts[case["name"]] = [len(mu) for mu, _ in sets]
        if max(counts[case["name"]]) > 64:
            (cut, _), _ = solve_case(case, sp, stream_limit=64)
            moved = [np.abs(full[c] - cut[c]).max() / scale for c in (4, 5, 6)]
            print(f"{case['name']}: streams {counts[case['name']]}, cut to 64 moves intralayer {moved[0]:.2e}, substrate {moved[1]:.2e}, "
                  f"interlayer {moved[2]:.2e}")
            assert moved[0] > 1000 * SIGMA_RTOL, (case["name"], moved)
            # the interlayer term stops at the shorter of two sets: it reads a stream past 64 only where both sets have one
            n = counts[case["name"]]
            if any(min(n[a], n[b]) > 64 for a in range(len(n)) for b in range(a + 1, len(n))):
                assert moved[2] > 1000 * SIGMA_RTOL, (case["name"], moved)
        k = case["m_max"]
        if case["name"].startswith("iba_exp_L2_go_m") and k in (4, 6, 7, 8):
            (less, _), _ = solve_case(dict(case, m_max=k - 1), sp)
            moved = [np.abs(full[c] - less[c]).max() / scale for c in (4, 5, 6)]
            print(f"{case['name']}: mode {k - 1} moves intralayer {moved[0]:.2e}, substrate {moved[1]:.2e}, interlayer {moved[2]:.2e}")
            assert moved[0] > 100 * SIGMA_RTOL and moved[1] > 100 * SIGMA_RTOL, (case["name"], moved)
    assert {n for n, c in counts.items() if max(c) > 64} == {"iba_exp_L2_n65_inter", "iba_exp_contrast_L3_n130_inter"}
    assert counts["iba_exp_L2_n64_inter"] == [47, 64] and counts["iba_exp_L2_n65_inter"] == [48, 65]
    assert counts["iba_exp_contrast_L3_n130_inter"] == [60, 130, 66] and counts["iba_exp_contrast_L3_go_n16_inter"] == [7, 16, 8]
    assert {by_name[f"iba_exp_L2_go_m{k}"]["m_max"] for k in (1, 4, 6, 7, 8)} == {1, 4, 6, 7, 8}
    # one layer with the interlayer option: the term is exactly zero
    assert not golden(by_name["iba_exp_L1_inter"])["contributions"][7].any()


EDGE_FREQUENCIES = (13e9, 17.25e9)
ST_INPUT = int(re.search(r"#define SMRT_ERR_INPUT\s+(\d+)", open(os.path.join(ROOT, "include", "smrt_dort.h")).read()).group(1))


@functools.lru_cache(maxsize=None)
def edge_batch(which):
    """The batches of the edge tests, as tuples of cases.
    "frequencies": 45 snowpacks of 1, 2, 3, 4, 1, .. layers for EDGE_FREQUENCIES x 3 angles (90 pairs, 270 items of the walk:
        a second block); two in three over a geometrical-optics soil whose mean square slope is the snowpack's own, the third
        over the Transparent substrate (its rows of the substrate table are zero).  Not Flat: a packed batch has ONE
        substrate kind (smrt_batch.substrate_kind; the solver groups snowpacks by it before it packs); these two are both
        evaluated by the caller, and the other rough soils refuse the bistatic modes this solver asks for.
    "streams": 8 snowpacks of 1 to 3 layers, densities 200 .. 850 kg m-3, n_max_stream 130, m_max 2.
    "two_streams": n_max_stream 2; the light layer of the middle snowpack keeps one of the two streams of the ice under it
        (relative sines 0.75 and 1.39)."""
    if which == "frequencies":
        def soil(k):
            return dict(transparent=True) if k % 3 == 2 else dict(substrate_model="geometrical_optics", mean_square_slope=0.02 + 0.002 * k, **R.SOIL)
        return tuple(random_batch(np.random.RandomState(23), [1, 2, 3, 4] * 11 + [1], [20.0, 35.0, 50.0], 6, 3, substrate=soil))
    if which == "streams":
        return tuple(random_batch(np.random.RandomState(33), [1, 2, 3, 2, 3, 3, 2, 3], [25.0, 40.0], 130, 2, density=(200.0, 850.0)))
    assert which == "two_streams"
    cases = random_batch(np.random.RandomState(3), [1, 2, 2], [25.0, 40.0], 2, 3)
    cases[1]["density"], cases[2]["density"] = [200.0, 850.0], [300.0, 320.0]
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def edge_group(which):
    return PackedGroup(edge_batch(which), EDGE_FREQUENCIES if which == "frequencies" else None)


@functools.lru_cache(maxsize=None)
def edge_reference(which):
    """The restatement on every global pair of edge_batch(which), at the pair's own frequency, interlayer term ON, computed
    once: a list of (contributions [7, n, 2, 2], backscatter_layer, stream counts per layer), read-only.  The interlayer
    option changes nothing but contribution 6 (second_order_restatement.second_order), so the reference with the option off
    is this one with that row zeroed: reference8()."""
    from smrt_amd.rtsolver.iterative_second_order import IterativeSecondOrder

    cases = edge_batch(which)
    sps = [build_snowpack(c, api()) for c in cases]
    out = []
    for f in (EDGE_FREQUENCIES if which == "frequencies" else (13e9,)):
        for case, sp in zip(cases, sps):
            layers = R.O.make_layers(case["emmodel"], f, R.oracle_snowpack(case))
            sets = IterativeSecondOrder.stream_sets(case["n_max_stream"], [complex(lay.eps_eff) for lay in layers])
            counts = tuple(len(mu) for mu, _ in sets)
            if min(counts) < 2:   # nothing to restate: the solver reports such a pair by its status
                out.append((None, None, counts))
                continue
            (c, pl), _ = solve_case(dict(case, frequency=f, interlayer=True), sp)
            c.setflags(write=False)
            pl.setflags(write=False)
            out.append((c, pl, counts))
    return out


def reference8(ref, interlayer):
    c = ref[0] if interlayer else np.concatenate([ref[0][:6], np.zeros_like(ref[0][6:])])
    return np.concatenate([c.sum(axis=0)[None], c])


def assert_batch_matches(out, cases, reference, interlayer, what):
    """Every global pair of a run of the whole batch against edge_reference; returns the worst error."""
    worst = 0.0
    assert len(out.values) == len(reference) and not out.status.any()
    for gp, ref in enumerate(reference):
        case = cases[gp % len(cases)]
        L = len(case["thickness"])
        worst = max(worst, assert_close(f"pair {gp}", case["theta"], out.values[gp], out.layer_backscatter[gp][:L + 1], reference8(ref, interlayer),
                                        ref[1], what))
        assert not out.layer_backscatter[gp][L + 1:].any()
        if not interlayer or L == 1:
            assert not out.values[gp][6].any()
    print(f"worst of the batch, {what}:", worst)
    return worst


def test_rough_pairs_of_the_frequency_batch_are_told_apart():
    """The input condition of the two-frequency batch: the order2_rough_layer_scattering rows of any two rough pairs differ
    by more than 1000 SIGMA_RTOL of the larger of their two scales, so a substrate row read at another pair's index -- the
    other frequency's, a neighbour's, the row of a chunk instead of the global pair -- cannot pass; the other pairs have none."""
    cases, ref = edge_batch("frequencies"), edge_reference("frequencies")
    S = len(cases)
    rough = [gp for gp in range(2 * S) if "transparent" not in cases[gp % S]["substrate"]]
    assert len(cases) == 45 and len(rough) == 60 and [len(c["thickness"]) for c in cases[:5]] == [1, 2, 3, 4, 1]
    for gp in set(range(2 * S)) - set(rough):
        assert not ref[gp][0][5].any()
    scale = {gp: scale_of(reference8(ref[gp], True)) for gp in rough}
    closest = min(np.abs(ref[a][0][5] - ref[b][0][5]).max() / max(scale[a], scale[b]) for a in rough for b in rough if a < b)
    print("closest two rough pairs:", closest)
    assert closest > 1000 * SIGMA_RTOL


@pytest.mark.parametrize("interlayer", [False, True], ids=["plain", "interlayer"])
def test_two_frequencies_and_rough_substrates_on_the_cpu(host_ctx, interlayer):
    """The whole two-frequency batch on the host build (which has neither chunks nor listed pairs: those are the GPU's)."""
    out = edge_group("frequencies").run(host_ctx, interlayer)
    assert_batch_matches(out, edge_batch("frequencies"), edge_reference("frequencies"), interlayer, "host build")


def assert_stream_counts_straddle(reference):
    counts = [n for ref in reference for n in ref[2]]
    assert min(counts) < 64 and any(64 < n < 128 for n in counts) and max(counts) > 128, counts
    # and inside one snowpack: the interlayer term stops at the shorter of two unequal sets on both sides of 64
    assert any(min(ref[2]) < 64 < max(ref[2]) for ref in reference), counts


def test_many_streams_in_a_batch_on_the_cpu(host_ctx):
    assert_stream_counts_straddle(edge_reference("streams"))
    out = edge_group("streams").run(host_ctx, True)
    assert_batch_matches(out, edge_batch("streams"), edge_reference("streams"), True, "host build, 130 streams")


def pack_c_abi(cases, interlayer, **struct_fields):
    """Cases packed for the C ABI, with nothing of the solver's host side in between."""
    from test_gpu_second_order import pack_batch

    batch, extras = pack_batch(list(cases), interlayer)
    for name, value in struct_fields.items():
        setattr(batch.struct, name, value)
    return batch, extras


def assert_one_stream_is_reported(out, first_values, first_layer_backscatter):
    """The outputs of edge_batch("two_streams"): the middle pair reports ST_INPUT, its order-2 rows are NaN and its
    first-order rows those of the first order, bit for bit."""
    assert ST_INPUT == 5 and "fewer than two streams" in _native.STATUS_MESSAGES[ST_INPUT]
    assert list(out.status) == [0, ST_INPUT, 0]
    assert np.isnan(out.values[1, 4:]).all() and np.isnan(out.layer_backscatter[1, 1:3]).all()
    assert np.array_equal(out.values[:, :4], first_values) and np.array_equal(out.layer_backscatter[1, 0], first_layer_backscatter[1, 0])
    for k in (0, 2):
        assert np.isfinite(out.values[k]).all() and np.isfinite(out.layer_backscatter[k]).all() and out.values[k, 4].all()


def test_a_layer_with_one_stream_is_reported_by_status_on_the_cpu(host_lib):
    """The light layer of the middle snowpack keeps one stream: ST_INPUT, NaN in the order-2 rows of that pair alone.  The
    first-order rows do not depend on the streams: those of the same batch with 8 streams, where no layer loses all but
    one."""
    from smrt_amd.rtsolver.iterative_second_order import IterativeSecondOrder

    eps = [[complex(lay.eps_eff) for lay in R.O.make_layers("iba", 13e9, R.oracle_snowpack(c))] for c in edge_batch("two_streams")]
    assert [[len(mu) for mu, _ in IterativeSecondOrder.stream_sets(2, e)] for e in eps] == [[2], [1, 2], [2, 2]]

    def run(batch, extras):
        o = _native.SecondOrderOutput(batch, batch.n_pairs)
        assert host_lib.smrt_second_order_host_run(C.byref(batch.struct), C.byref(extras.struct), 0, *o.pointers()) == 0
        return o

    out = run(*pack_c_abi(edge_batch("two_streams"), True))
    eight = run(*pack_c_abi(edge_batch("two_streams"), True, n_max_stream=8))
    assert not eight.status.any() and np.isfinite(eight.values).all()
    assert_one_stream_is_reported(out, eight.values[:, :4], eight.layer_backscatter)


EDGE_ANGLE_CASE = "iba_exp_contrast_L3_go_n16_inter"


def assert_common_angle_is_the_same(run):
    """`run(case)` -> output of one pair.  The case with its angles, with 40 degrees alone and with five angles of which 40
    degrees is the fourth: a unit decoded by `unit % n_theta` lands on the same numbers whatever n_theta is."""
    case = next(c for c in CASES if c["name"] == EDGE_ANGLE_CASE)
    assert case["theta"][1] == 40.0
    two, one, five = run(case), run(dict(case, theta=[40.0])), run(dict(case, theta=[10.0, 25.0, 55.0, 40.0, 70.0]))
    assert one.status[0] == 0 and five.status[0] == 0 and one.values[0, 5].all() and one.values[0, 6].all()
    for other, t in ((two, 1), (five, 3)):
        assert np.array_equal(one.values[0][:, 0], other.values[0][:, t])
        assert np.array_equal(one.layer_backscatter[0][:, 0], other.layer_backscatter[0][:, t])


def test_the_common_angle_does_not_depend_on_the_angle_count_on_the_cpu(host_ctx):
    assert_common_angle_is_the_same(lambda case: run_case(case, host_ctx))
