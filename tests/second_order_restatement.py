"""NumPy restatement of the iterative second-order backscatter solution (Karam et al. 1995, eqs. A8, A11, A13; azimuth
integral by Fourier modes as in Tsang et al. 2007, appendix 2) and the case table of the fixtures
tests/golden/second_order_*.npz.  Orders 0 and 1 are the first-order restatement (tests/first_order_restatement.py); this
file adds the three order-2 mechanisms.  It stands in for the reference where the reference does not exist (the GPU
tests): tests/test_second_order_cpu.py holds it to every fixture.

Each order-2 term is, per layer n and incidence angle, a quadrature over the layer's stream cosines mu' (the layer's
stream set, ascending) of

    coefficient(mu_n, mu') x  sum_m w_m  M1_m M2_m            w_0 = 2 pi,  w_m = pi cos(m pi), m = 1 .. m_max - 1

with M1, M2 azimuth modes (3 polarisations) of two phase matrices / 4 pi -- or of the substrate's diffuse reflection and one
phase matrix --, applied to the downward intensity in the layer and carried to the air by the cumulative upward
transmission.  Only the V, H block of the product is formed: the incident beam has no third Stokes component, the
interfaces are diagonal, and the result is cut to V, H.

Written as the reference computes, oddities included: mode m_max is never summed; the interlayer term pairs the i-th
stream of layer n with the i-th of layer m, stops at the shorter set, weights with layer n's weights, evaluates every
attenuation factor with layer n's cosines, starts its second-layer loop at layer 1, and its intermediate optical depth
contains both end layers (the term can be negative).  The one deliberate difference: where a stream cosine equals the
incidence cosine exactly the reference's coefficients are 0 / 0; here they take their analytic limit (D, which has a simple
pole there, the finite part of its Laurent expansion = the limit of the mean of its two neighbours).
"""
import numpy as np

from oracle import dort_oracle as O

import first_order_restatement as FO
from first_order_restatement import SIGMA_RTOL, build_snowpack, oracle_snowpack, snell_from_air  # noqa: F401

CONTRIBUTIONS = FO.CONTRIBUTIONS + ["order2_intralayer_scattering", "order2_rough_layer_scattering",
                                    "order2_interlayer_scattering"]

SOIL = dict(permittivity_model=complex(8.0, 1.0), temperature=268.0)
GO_SOIL = dict(substrate_model="geometrical_optics", mean_square_slope=0.05, **SOIL)
_L3 = dict(frequency=13e9, thickness=[0.3, 0.4, 0.6], density=[250.0, 400.0, 300.0], temperature=[258.0, 261.0, 264.0],
           microstructure_model="exponential", corr_length=[2e-4, 3e-4, 4e-4], emmodel="iba")
CASES = [
    dict(name="iba_exp_L1_m2", emmodel="iba", frequency=17.25e9, theta=[20.0, 40.0], thickness=[1000.0], density=[320.0],
         temperature=[260.0], microstructure_model="exponential", corr_length=[2e-4], n_max_stream=8, m_max=2),
    dict(name="iba_exp_L1_defaults", emmodel="iba", frequency=17.25e9, theta=[35.0], thickness=[1000.0], density=[320.0],
         temperature=[260.0], microstructure_model="exponential", corr_length=[2e-4], n_max_stream=32, m_max=5),
    dict(name="iba_exp_L3_flat", theta=[20.0, 35.0, 50.0], substrate=dict(substrate_model="flat", **SOIL), n_max_stream=8,
         m_max=3, **_L3),
    dict(name="iba_exp_L3_go", theta=[20.0, 35.0, 50.0], substrate=GO_SOIL, n_max_stream=8, m_max=3, **_L3),
    dict(name="iba_exp_L3_go_inter", theta=[25.0, 40.0], substrate=GO_SOIL, n_max_stream=8, m_max=3, interlayer=True, **_L3),
    dict(name="iba_exp_L2_inter", emmodel="iba", frequency=13e9, theta=[30.0], thickness=[0.4, 0.8], density=[300.0, 300.0],
         temperature=[260.0, 262.0], microstructure_model="exponential", corr_length=[3e-4, 4e-4],
         substrate=dict(substrate_model="flat", **SOIL), n_max_stream=6, m_max=3, interlayer=True),
    dict(name="qca_shs_L3_flat", emmodel="dmrt_qca_shortrange", frequency=13.4e9, theta=[20.0, 45.0], thickness=[0.2, 0.3, 0.6],
         density=[200.0, 280.0, 330.0], temperature=[258.0, 261.0, 264.0], microstructure_model="sticky_hard_spheres",
         radius=[3e-4, 4e-4, 5e-4], stickiness=[0.2, 0.3, 0.4], substrate=dict(substrate_model="flat", **SOIL), n_max_stream=8,
         m_max=3, interlayer=True),
    dict(name="rayleigh_L2_flat", emmodel="rayleigh", frequency=13.4e9, theta=[30.0, 50.0], thickness=[0.3, 0.7],
         density=[250.0, 320.0], temperature=[260.0, 263.0], microstructure_model="independent_sphere", radius=[4e-4, 5e-4],
         substrate=dict(substrate_model="flat", **SOIL), n_max_stream=8, m_max=3),
    dict(name="iba_exp_wet_L3_flat", emmodel="iba", frequency=5.405e9, theta=[20.0, 45.0], thickness=[0.05, 0.3, 0.6],
         density=[300.0, 320.0, 350.0], temperature=[273.15, 270.0, 268.0], microstructure_model="exponential",
         corr_length=[3e-4, 2e-4, 2e-4], volumetric_liquid_water=[0.02, 0.0, 0.0], substrate=dict(substrate_model="flat", **SOIL),
         n_max_stream=8, m_max=3),
    dict(name="mixed_L3_flat", emmodel=["iba", "nonscattering", "dmrt_qca_shortrange"], frequency=17.25e9, theta=[25.0, 40.0],
         thickness=[0.15, 0.25, 0.5], density=[230.0, 290.0, 340.0], temperature=[257.0, 260.0, 263.0],
         microstructure_model="sticky_hard_spheres", radius=[3e-4, 3e-4, 4e-4], stickiness=[0.2, 0.3, 0.4],
         substrate=dict(substrate_model="flat", **SOIL), n_max_stream=8, m_max=3, interlayer=True),
    dict(name="iba_exp_transparent_L2", emmodel="iba", frequency=13e9, theta=[30.0, 40.0], thickness=[0.5, 2.0],
         density=[280.0, 320.0], temperature=[260.0, 262.0], microstructure_model="exponential", corr_length=[2e-4, 3e-4],
         substrate=dict(transparent=True), n_max_stream=8, m_max=3),
    dict(name="iba_exp_iem_surface_L3", emmodel="iba", frequency=13.4e9, theta=[20.0, 40.0], thickness=[0.3, 0.25, 0.8],
         density=[250.0, 300.0, 350.0], temperature=[258.0, 261.0, 264.0], microstructure_model="exponential",
         corr_length=[2e-4, 2.5e-4, 3e-4], interfaces=[FO.IEM, None, None], substrate=dict(substrate_model="flat", **SOIL),
         n_max_stream=8, m_max=3),
]

# ---- the edge cases: shapes at which the device's own choices (streams on 64 lanes, the mode table of M in {2, 3, 5, 8}
# registers, substrate rows per stream) take another path.  tests/test_second_order_cpu.py:test_edge_fixtures_are_sensitive
# holds each to the condition that makes it able to fail.
FLAT_SOIL = dict(substrate_model="flat", **SOIL)
_L2 = dict(emmodel="iba", frequency=13e9, theta=[25.0, 40.0], thickness=[0.4, 0.8], density=[250.0, 380.0],
           temperature=[260.0, 262.0], microstructure_model="exponential", corr_length=[3e-4, 8e-4])
# a light layer, nearly solid ice, a light layer: the ice keeps every stream, its neighbours lose about half of theirs; coarse
# enough below the top layer for the streams past the 64th to carry more than 1000 SIGMA_RTOL of the total
_CONTRAST = dict(emmodel="iba", frequency=13e9, theta=[25.0, 40.0], thickness=[0.3, 0.2, 0.5], density=[200.0, 850.0, 300.0],
                 temperature=[258.0, 261.0, 264.0], microstructure_model="exponential", corr_length=[3e-4, 1e-3, 8e-4])
# thin layers of coarse grains at 37 GHz over a smooth rough soil, steep incidence: azimuth modes up to 7 are all above
# 100 SIGMA_RTOL of the total in the intralayer and the substrate terms (the figures: test_edge_fixtures_are_sensitive)
_MODES = dict(emmodel="iba", frequency=37e9, theta=[40.0, 60.0], thickness=[0.01, 0.01], density=[250.0, 380.0],
              temperature=[258.0, 262.0], microstructure_model="exponential", corr_length=[1e-3, 1.5e-3],
              substrate=dict(substrate_model="geometrical_optics", mean_square_slope=0.003, **SOIL), n_max_stream=8,
              interlayer=True)
_RAYLEIGH = next(dict(c) for c in CASES if c["name"] == "rayleigh_L2_flat")
EDGE_CASES = [
    dict(name="iba_exp_L2_n64_inter", substrate=FLAT_SOIL, n_max_stream=64, m_max=3, interlayer=True, **_L2),
    dict(name="iba_exp_L2_n65_inter", substrate=FLAT_SOIL, n_max_stream=65, m_max=3, interlayer=True, **_L2),
    dict(name="iba_exp_contrast_L3_n130_inter", substrate=FLAT_SOIL, n_max_stream=130, m_max=2, interlayer=True, **_CONTRAST),
    dict(name="iba_exp_contrast_L3_go_n16_inter", substrate=GO_SOIL, n_max_stream=16, m_max=3, interlayer=True, **_CONTRAST),
] + [dict(name=f"iba_exp_L2_go_m{k}", m_max=k, **_MODES) for k in (1, 4, 6, 7, 8)] + [
    dict(_RAYLEIGH, name="rayleigh_L2_flat_m8", m_max=8),
    dict(_RAYLEIGH, name="rayleigh_L2_flat_m2", m_max=2),
    dict(name="iba_exp_L1_inter", emmodel="iba", frequency=13e9, theta=[25.0, 40.0], thickness=[0.6], density=[300.0],
         temperature=[260.0], microstructure_model="exponential", corr_length=[3e-4], substrate=FLAT_SOIL, n_max_stream=8, m_max=3,
         interlayer=True),
]
EDGE_NAMES = [c["name"] for c in EDGE_CASES]
CASES += EDGE_CASES


def options_of(case):
    return dict(n_max_stream=case["n_max_stream"], m_max=case["m_max"],
                compute_scattering_interlayer=bool(case.get("interlayer", False)))


# ---- the closed-form factors (any float type: the tests evaluate them in np.longdouble) --------------------------------
def _g(mu, tau):
    return np.exp(-tau / mu)


def coef_A(mu_i, mu, ke, tau):
    gi, gm = _g(mu_i, tau), _g(mu, tau)
    ratio = -tau * gi if mu == mu_i else (gi - gm) / (1 / mu_i - 1 / mu)       # (g(mu_i) - g(mu)) / (1/mu_i - 1/mu)
    return gi * (ratio / ke + mu_i / (2 * ke) * (1 - gi ** 2)) / (ke * (mu_i + mu))


def coef_B(mu_i, mu, ke, tau):
    gi, gm = _g(mu_i, tau), _g(mu, tau)
    ratio = -tau * gi if mu == mu_i else (gm - gi) / (1 / mu - 1 / mu_i)
    return (mu_i * (1 - gi ** 2) / (2 * ke) + gi * ratio / ke) / (ke * (mu + mu_i))


def coef_C(mu_i, mu, ke_n, ke_m, tau_n, tau_m, tau_r):
    gin, gim, gmn, gmm = _g(mu_i, tau_n), _g(mu_i, tau_m), _g(mu, tau_n), _g(mu, tau_m)
    ratio = -tau_m * gim if mu == mu_i else (gmm - gim) / (1 / mu - 1 / mu_i)
    return gmn * (1 - gin * gmn) / (ke_n * (mu + mu_i)) * ratio / ke_m * _g(mu_i, tau_r) * _g(mu, tau_r)


def coef_D(mu_i, mu, ke_n, ke_m, tau_n, tau_m, tau_r):
    gin, gim = _g(mu_i, tau_n), _g(mu_i, tau_m)
    if mu == mu_i:
        # D = F(mu) G(mu) / (mu_i - mu)^2 with F = g_m(mu_i) - g_m(mu) -> 0 and G regular: a simple pole.  Its finite part
        # -(F'' G / 2 + F' G') at mu_i, F' / F'' the derivatives of g_m = exp(-tau_m / mu)
        a, gr = mu_i, _g(mu_i, tau_r)
        k = gim * gr / (ke_n * ke_m)
        f1 = gim * tau_m / a ** 2
        f2 = gim * (tau_m ** 2 / a ** 4 - 2 * tau_m / a ** 3)
        G = k * a ** 2 * (1 - gin ** 2) * gr
        G1 = k * a * gr * ((1 - gin ** 2) - gin ** 2 * tau_n / a + (1 - gin ** 2) * tau_r / a)
        return -(f2 * G / 2 + f1 * G1)
    gmn, gmm = _g(mu, tau_n), _g(mu, tau_m)
    return ((gim - gmm) / (ke_m * (mu_i - mu)) * gim * (1 - gmn * gin) / (ke_n * (1 / mu - 1 / mu_i))
            * _g(mu_i, tau_r) * _g(mu, tau_r))


def coef_F(mu_i, mu, ke, tau, tau_ground):
    gi, gm = _g(mu_i, tau), _g(mu, tau)
    ratio = gi * tau / mu_i ** 2 if mu == mu_i else (gm - gi) / (mu - mu_i)
    return gi * mu_i * ratio / ke * _g(mu_i, tau_ground) * _g(mu, tau_ground)


def coef_E(mu_i, mu, ke, tau, tau_ground):
    return _g(mu_i, tau) * coef_F(mu_i, mu, ke, tau, tau_ground)


# ---- azimuth modes -----------------------------------------------------------------------------------------------------
def layer_modes(layer, mu_s, mu_i, m_max):
    """[3, 3, m_max + 1] azimuth modes of the phase matrix / 4 pi of an oracle layer between two cosines."""
    if layer.ks == 0.0:
        return np.zeros((3, 3, m_max + 1))
    p = layer.ft_even_phase(np.array([mu_s]), np.array([mu_i]), m_max, 3)
    return np.asarray(p, float)[:, :, :, 0, 0] / (4 * np.pi)


def mode_sum(m1, m2, m_max):
    """V, H block of sum_m w_m m1[:, :, m] @ m2[:, :, m], m < m_max."""
    out = 2 * np.pi * (m1[:, :, 0] @ m2[:, :, 0])
    for m in range(1, m_max):
        out = out + np.pi * np.cos(m * np.pi) * (m1[:, :, m] @ m2[:, :, m])
    return out[:2, :2]


def substrate_modes(substrate, frequency, eps_last, mu_i, mu, m_max):
    """The two samples of the substrate's diffuse reflection modes the substrate term reads, [3, 3, m_max + 1] each:
    R(-mu_i <- mu') and R(mu' <- mu_i), through the protocol with the symmetric cosine vectors the solver hands over."""
    a, b = np.array([-mu_i, mu_i]), np.array([-mu, mu])
    r1 = substrate.ft_even_diffuse_reflection_matrix(frequency, eps_last, a, b, m_max, 3)
    r2 = substrate.ft_even_diffuse_reflection_matrix(frequency, eps_last, b, a, m_max, 3)
    r1, r2 = (np.asarray(getattr(r, "values", r), float) for r in (r1, r2))
    if r1.ndim == 0 and r2.ndim == 0 and r1 == 0.0 and r2 == 0.0:   # a substrate without diffuse reflection (Transparent)
        return np.zeros((3, 3, m_max + 1)), np.zeros((3, 3, m_max + 1))
    return r1[:, :, :, 0, 1], r2[:, :, :, 1, 1]


def has_diffuse_modes(obj):
    return obj is not None and not isinstance(obj, tuple) and callable(getattr(obj, "ft_even_diffuse_reflection_matrix", None))


# ---- the solution ------------------------------------------------------------------------------------------------------
def second_order(layers, thickness, frequency, theta_deg, interfaces=None, substrate=None, n_max_stream=32, m_max=5,
                 interlayer=False, stream_limit=None):
    """(contributions [7, n, 2, 2], backscatter_layer [L + 1, n, 2, 2]) for oracle layers.  `stream_limit` (tests only):
    every layer's stream set, ascending, is cut to its first `stream_limit` entries AFTER the weights are made -- what a
    wavefront computes whose lanes never take a second trip over the streams."""
    L = len(layers)
    first, per_layer1 = FO.first_order(layers, thickness, frequency, theta_deg, interfaces, substrate)
    theta = np.deg2rad(np.atleast_1d(np.asarray(theta_deg, float)))
    out = np.zeros((7, len(theta), 2, 2))
    out[:4] = first
    per_layer = per_layer1.copy()
    interfaces = interfaces or [None] * L
    eps = [1.0 + 0j] + [complex(lay.eps_eff) for lay in layers]
    st = O.compute_streams(n_max_stream, np.array(eps[1:]))
    smu = [m[::-1][:stream_limit] for m in st.mu]
    sw = [w[::-1][:stream_limit] for w in st.weight]
    ke = [lay.ks + lay.ka for lay in layers]
    tau = [k * d for k, d in zip(ke, thickness)]
    rough = has_diffuse_modes(substrate)
    for t, mu0 in enumerate(np.cos(theta)):
        mu = [mu0] + [snell_from_air(e, mu0) for e in eps[1:]]
        bnd = [FO.boundary(interfaces[k], frequency, eps[k], eps[k + 1], mu[k], mu[k + 1]) for k in range(L)]
        down = np.diag(bnd[0][1]) * (1.0 / eps[1].real) * (mu0 / mu[1])
        up = np.ones(2)
        acc = np.zeros((2, 2, 2))   # intra, ground: running sums (backscatter_layer is cumulative, as the reference's)
        for n in range(L):
            lay, mi = layers[n], mu[n + 1]
            up = up * bnd[n][2]
            U = np.diag(up)
            s_intra, s_ground = np.zeros((2, 2)), np.zeros((2, 2))
            for x, w in zip(smu[n], sw[n]):
                s_intra += w * coef_A(mi, x, ke[n], tau[n]) * mode_sum(layer_modes(lay, mi, x, m_max), layer_modes(lay, x, -mi, m_max), m_max)
                s_intra += w * coef_B(mi, x, ke[n], tau[n]) * mode_sum(layer_modes(lay, mi, -x, m_max), layer_modes(lay, -x, -mi, m_max), m_max)
                if rough:
                    tg = sum(tau[n:])
                    r1, r2 = substrate_modes(substrate, frequency, eps[L], mi, x, m_max)
                    s_ground += w * coef_E(mi, x, ke[n], tau[n], tg) * mode_sum(r1, layer_modes(lay, -x, -mi, m_max), m_max)
                    s_ground += w * coef_F(mi, x, ke[n], tau[n], tg) * mode_sum(r2, layer_modes(lay, mi, x, m_max), m_max)
            out[4, t] += U @ s_intra @ down
            out[5, t] += U @ s_ground @ down
            acc = acc + np.array([U @ s_intra @ down, U @ s_ground @ down])
            per_layer[n + 1, t] += (acc[0] + acc[1]) * mi * 4 * np.pi
            if interlayer:
                tau_r = tau[n]
                for m in range(max(n + 1, 1), L):
                    tau_r += tau[m]
                    s = np.zeros((2, 2))
                    for x, w, y in zip(smu[n], sw[n], smu[m]):
                        c = coef_C(mi, x, ke[n], ke[m], tau[n], tau[m], tau_r)
                        d = coef_D(mi, x, ke[n], ke[m], tau[n], tau[m], tau_r)
                        mm = mu[m + 1]
                        s += w * c * mode_sum(layer_modes(lay, mi, x, m_max), layer_modes(layers[m], y, -mm, m_max), m_max)
                        s += w * d * mode_sum(layer_modes(layers[m], mm, -y, m_max), layer_modes(lay, -x, -mi, m_max), m_max)
                    out[6, t] += U @ s @ down
            if n < L - 1:
                two_way = np.exp(-2.0 * tau[n] / mi)
                down = np.diag(bnd[n + 1][1]) @ (two_way * (eps[n + 1].real / eps[n + 2].real) * (mi / mu[n + 2]) * down)
    return out, per_layer


def solve_case(case, snowpack, emmodel_names=None, stream_limit=None):
    """The restatement on a fixture case; `snowpack`: the package's Snowpack built by build_snowpack."""
    wet = None
    if "volumetric_liquid_water" in case:
        wet = ([float(getattr(lay, "liquid_water", 0) or 0) for lay in snowpack.layers], [lay.frac_volume for lay in snowpack.layers])
    layers = O.make_layers(emmodel_names or case["emmodel"], case["frequency"], oracle_snowpack(case, wet))
    interfaces = [None if type(i).__name__ == "Flat" else i for i in snowpack.interfaces]
    sub, spec = snowpack.substrate, case.get("substrate")
    if spec and spec.get("substrate_model") == "flat":
        sub = ("flat", spec["permittivity_model"])
    return second_order(layers, case["thickness"], case["frequency"], case["theta"], interfaces, sub, case["n_max_stream"],
                        case["m_max"], bool(case.get("interlayer")), stream_limit), layers
