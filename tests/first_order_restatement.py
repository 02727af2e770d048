"""NumPy restatement of the iterative first-order backscatter solution, written from the equations (Ulaby et al. 2014,
eqs. 11.62, 11.74, 11.75; refraction factor of Tsang et al. 2007, eqs. 22a/b), and the case table of the fixtures
tests/golden/first_order_*.npz.  It stands in for the reference where the reference does not exist (the GPU tests):
tests/test_first_order_cpu.py holds it to every fixture.

Layer scalars and phase functions come from the project's CPU oracle (oracle/dort_oracle.py); Flat interfaces are Fresnel;
any other interface / substrate is an object that speaks the interface protocol and is evaluated at (mu, mu, pi).
"""
import numpy as np

from oracle import dort_oracle as O

CONTRIBUTIONS = ["total", "order0_backscatter", "order1_direct_backscatter", "order1_double_bounce",
                 "order1_reflected_backscatter"]
SIGMA_RTOL = 1e-8   # of the solve's largest co-polarised total: the project's bar for sigma0 against the reference

# ---- the fixtures ----------------------------------------------------------------------------------------------------
_L30 = np.random.RandomState(7)
IEM = ("iem_fung92", dict(roughness_rms=0.002, corr_length=0.05))
GOB = ("geometrical_optics_backscatter", dict(mean_square_slope=0.03))
SOIL = dict(permittivity_model=complex(8.0, 1.0), temperature=268.0)
CASES = [
    dict(name="iba_exp_L1_none", emmodel="iba", frequency=17.25e9, theta=[20.0, 30.0, 45.0], thickness=[1000.0],
         density=[320.0], temperature=[260.0], microstructure_model="exponential", corr_length=[2e-4]),
    dict(name="iba_exp_L3_flat", emmodel="iba", frequency=13.4e9, theta=[5.0, 25.0, 40.0, 55.0, 70.0], thickness=[0.2, 0.3, 0.5],
         density=[220.0, 300.0, 380.0], temperature=[255.0, 260.0, 265.0], microstructure_model="exponential",
         corr_length=[1e-4, 2e-4, 3e-4], substrate=dict(substrate_model="flat", **SOIL)),
    dict(name="iba_shs_L3_reflector", emmodel="iba", frequency=17.25e9, theta=[20.0, 35.0, 50.0], thickness=[0.1, 0.2, 0.4],
         density=[250.0, 300.0, 350.0], temperature=[258.0, 261.0, 264.0], microstructure_model="sticky_hard_spheres",
         radius=[2e-4, 3e-4, 4e-4], stickiness=[0.2, 0.3, 0.5], substrate=dict(reflector=dict(V=0.6, H=0.7))),
    dict(name="qca_shs_L3_iem", emmodel="dmrt_qca_shortrange", frequency=13.4e9, theta=[20.0, 30.0, 45.0],
         thickness=[0.2, 0.3, 0.6], density=[200.0, 280.0, 330.0], temperature=[258.0, 261.0, 264.0],
         microstructure_model="sticky_hard_spheres", radius=[2e-4, 3e-4, 3.5e-4], stickiness=[0.2, 0.3, 0.4],
         substrate=dict(substrate_model="iem_fung92", roughness_rms=0.004, corr_length=0.05, **SOIL)),
    dict(name="nonscattering_L2_gob", emmodel="nonscattering", frequency=5.405e9, theta=[10.0, 20.0, 30.0], thickness=[0.3, 0.7],
         density=[300.0, 400.0], temperature=[262.0, 266.0], microstructure_model="exponential", corr_length=[1e-4, 1e-4],
         substrate=dict(substrate_model="geometrical_optics_backscatter", mean_square_slope=0.05, **SOIL)),
    dict(name="mixed_L3_flat", emmodel=["iba", "dmrt_qca_shortrange", "nonscattering"], frequency=17.25e9,
         theta=[25.0, 40.0], thickness=[0.15, 0.25, 0.5], density=[230.0, 290.0, 340.0], temperature=[257.0, 260.0, 263.0],
         microstructure_model="sticky_hard_spheres", radius=[2e-4, 3e-4, 3e-4], stickiness=[0.2, 0.3, 0.4],
         substrate=dict(substrate_model="flat", **SOIL)),
    dict(name="iba_exp_wet_L3_flat", emmodel="iba", frequency=5.405e9, theta=[20.0, 33.0, 45.0], thickness=[0.05, 0.3, 0.6],
         density=[300.0, 320.0, 350.0], temperature=[273.15, 270.0, 268.0], microstructure_model="exponential",
         corr_length=[3e-4, 2e-4, 2e-4], volumetric_liquid_water=[0.02, 0.0, 0.0], substrate=dict(substrate_model="flat", **SOIL)),
    dict(name="iba_exp_L30_flat", emmodel="iba", frequency=5.405e9, theta=[20.0, 25.0, 30.0, 35.0, 40.0, 45.0],
         thickness=list(_L30.uniform(0.02, 0.1, 30)), density=list(_L30.uniform(150.0, 450.0, 30)),
         temperature=list(_L30.uniform(250.0, 270.0, 30)), microstructure_model="exponential",
         corr_length=list(_L30.uniform(5e-5, 4e-4, 30)), substrate=dict(substrate_model="flat", **SOIL)),
    dict(name="iba_exp_thin_L3_none", emmodel="iba", frequency=37e9, theta=[30.0, 50.0], thickness=[0.001, 0.2, 50.0],
         density=[150.0, 280.0, 350.0], temperature=[255.0, 260.0, 265.0], microstructure_model="exponential",
         corr_length=[1e-4, 2e-4, 2.5e-4]),
    dict(name="iba_exp_rough_L3_flat", emmodel="iba", frequency=13.4e9, theta=[20.0, 30.0, 40.0], thickness=[0.3, 0.25, 0.8],
         density=[250.0, 300.0, 350.0], temperature=[258.0, 261.0, 264.0], microstructure_model="exponential",
         corr_length=[1e-4, 1.5e-4, 2e-4], interfaces=[GOB, None, IEM], substrate=dict(substrate_model="flat", **SOIL)),
    dict(name="iba_exp_transparent_L2", emmodel="iba", frequency=13e9, theta=[30.0, 40.0], thickness=[0.5, 1000.0],
         density=[280.0, 320.0], temperature=[260.0, 262.0], microstructure_model="exponential", corr_length=[2e-4, 3e-4],
         interfaces=[("transparent", {}), ("transparent", {})], substrate=dict(transparent=True)),
]
# the example of the solver's documentation: make_model("iba", "iterative_first_order") on the IBA / exponential snowpacks
EXAMPLE_CASES = ["iba_exp_L1_none"]


def build_snowpack(case, api):
    """The snowpack of a case with the constructors of `api` (the package under test, or the reference: the two share the
    names make_snowpack, make_interface, make_soil; api.make_reflector / api.transparent_substrate are looked up by the
    caller)."""
    kw = {k: case[k] for k in ("temperature", "corr_length", "radius", "stickiness", "volumetric_liquid_water") if k in case}
    interfaces = None
    if case.get("interfaces"):
        interfaces = [api.make_interface("flat") if i is None else api.make_interface(i[0], **i[1]) for i in case["interfaces"]]
    sub = case.get("substrate")
    substrate = None
    if sub and "reflector" in sub:
        substrate = api.make_reflector(specular_reflection=dict(sub["reflector"]))
    elif sub and "transparent" in sub:
        substrate = api.transparent_substrate()
    elif sub:
        substrate = api.make_soil(**sub)
    return api.make_snowpack(case["thickness"], case["microstructure_model"], density=case["density"], interface=interfaces,
                             substrate=substrate, **kw)


def oracle_snowpack(case, liquid_water=None):
    """The dict of arrays oracle.make_layers reads."""
    sp = dict(thickness=np.asarray(case["thickness"], float), density=np.asarray(case["density"], float),
              temperature=np.asarray(case["temperature"], float), microstructure=case["microstructure_model"])
    for k in ("corr_length", "radius", "stickiness"):
        if k in case:
            sp[k] = np.asarray(case[k], float)
    if liquid_water is not None:
        sp["liquid_water"], sp["frac_volume"] = np.asarray(liquid_water[0], float), np.asarray(liquid_water[1], float)
    return sp


# ---- the solution ----------------------------------------------------------------------------------------------------
def snell_from_air(eps, mu0):
    eps = complex(eps)
    return np.sqrt(eps - (1.0 - mu0 ** 2) + 0j).real / np.sqrt(eps).real


def layer_phase(layer, mu_s, mu_i):
    """2 x 2 phase matrix [scattered, incident] of an oracle layer at azimuth pi."""
    if layer.ks == 0.0:
        return np.zeros((2, 2))
    if hasattr(layer, "iba_coeff"):
        return np.asarray(layer.phase(mu_s, mu_i, np.pi, 2), float)[:, :, 0, 0, 0]
    p, _ = O.rayleigh_matrix_and_half_angle(mu_s, mu_i, np.pi, 2)
    return 1.5 * layer.ks * p[:, :, 0, 0, 0]


def _rows(v, n):
    a = np.asarray(getattr(v, "values", v), float)
    return np.full((2, n), float(a)) if a.ndim == 0 else a[:2]


def _diffuse(v):
    a = np.asarray(getattr(v, "values", v), float)
    if a.ndim == 0:
        return np.zeros((2, 2))
    if a.ndim == 5:
        return a[:2, :2, 0, 0, 0]
    return np.diag(a[:2, 0])


def boundary(obj, frequency, e_above, e_below, mu_above, mu_below, substrate=None):
    """(R[2], T_down[2], T_up[2], D[2, 2]) of the boundary under a medium: `obj` an interface object (None: Flat) towards
    e_below, or -- e_below None -- what lies under the last layer: `substrate` None, ("flat", eps), ("reflector", rv, rh) or
    an object with the substrate protocol."""
    mu = np.array([mu_above])
    if e_below is None:
        if substrate is None:
            return np.zeros(2), np.zeros(2), np.zeros(2), np.zeros((2, 2))
        if isinstance(substrate, tuple) and substrate[0] == "flat":
            return O.flat_reflection(e_above, substrate[1], mu, 2)[:, 0], np.zeros(2), np.zeros(2), np.zeros((2, 2))
        if isinstance(substrate, tuple):
            return np.array(substrate[1:3], float), np.zeros(2), np.zeros(2), np.zeros((2, 2))
        r = _rows(substrate.specular_reflection_matrix(frequency, e_above, mu, 2), 1)[:, 0]
        d = np.zeros((2, 2))
        if callable(getattr(substrate, "diffuse_reflection_matrix", None)):
            d = _diffuse(substrate.diffuse_reflection_matrix(frequency, e_above, mu, mu, np.pi, 2))
        return r, np.zeros(2), np.zeros(2), d
    if obj is None:
        r = O.flat_reflection(e_above, e_below, mu, 2)[:, 0]
        r_up = O.flat_reflection(e_below, e_above, np.array([mu_below]), 2)[:, 0]
        return r, 1.0 - r, 1.0 - r_up, np.zeros((2, 2))
    r = _rows(obj.specular_reflection_matrix(frequency, e_above, e_below, mu, 2), 1)[:, 0]
    t_dn = _rows(obj.coherent_transmission_matrix(frequency, e_above, e_below, mu, 2), 1)[:, 0]
    t_up = _rows(obj.coherent_transmission_matrix(frequency, e_below, e_above, np.array([mu_below]), 2), 1)[:, 0]
    d = np.zeros((2, 2))
    if callable(getattr(obj, "diffuse_reflection_matrix", None)):
        d = _diffuse(obj.diffuse_reflection_matrix(frequency, e_above, e_below, mu, mu, np.pi, 2))
    return r, t_dn, t_up, d


def first_order(layers, thickness, frequency, theta_deg, interfaces=None, substrate=None):
    """(contributions [4, n, 2, 2], backscatter_layer [L + 1, n, 2, 2]) for oracle layers (eps_eff, ks, ka, phase)."""
    L = len(layers)
    theta = np.deg2rad(np.atleast_1d(np.asarray(theta_deg, float)))
    out = np.zeros((4, len(theta), 2, 2))
    per_layer = np.zeros((L + 1, len(theta), 2, 2))
    interfaces = interfaces or [None] * L
    eps = [1.0 + 0j] + [complex(lay.eps_eff) for lay in layers]
    for t, mu0 in enumerate(np.cos(theta)):
        mu = [mu0] + [snell_from_air(e, mu0) for e in eps[1:]]
        # boundaries[k]: under medium k (0: the air), i.e. the interface on top of layer k, or the substrate for k = L
        bnd = [boundary(interfaces[k], frequency, eps[k], eps[k + 1], mu[k], mu[k + 1]) for k in range(L)]
        bnd.append(boundary(None, frequency, eps[L], None, mu[L], None, substrate=substrate))
        out[0, t] = bnd[0][3]
        per_layer[0, t] = bnd[0][3] * mu0 * 4 * np.pi
        down = np.diag(bnd[0][1]) * (1.0 / eps[1].real) * (mu0 / mu[1])      # intensity entering layer 1 per unit incident
        up = np.ones(2)
        for l in range(1, L + 1):
            lay, d = layers[l - 1], thickness[l - 1]
            up = up * bnd[l - 1][2]
            r, t_dn, _, diffuse = bnd[l]
            ke = lay.ks + lay.ka
            m = mu[l]
            two_way = np.exp(-2.0 * ke * d / m)
            source = -np.expm1(-2.0 * ke * d / m) / (2.0 * ke)
            R, U = np.diag(r), np.diag(up)
            p_back = layer_phase(lay, -m, m) / (4 * np.pi)
            p_down = layer_phase(lay, m, -m) / (4 * np.pi)
            p_fwd_up = layer_phase(lay, m, m) / (4 * np.pi)
            p_fwd_dn = layer_phase(lay, -m, -m) / (4 * np.pi)
            terms = [U @ (two_way * diffuse) @ down,
                     U @ (source * p_back) @ down,
                     U @ (d * two_way / m * (p_fwd_dn @ R + R @ p_fwd_up)) @ down,
                     U @ (source * two_way * (R @ p_down @ R)) @ down]
            for c in range(4):
                out[c, t] += terms[c]
            per_layer[l, t] = sum(terms) * m * 4 * np.pi
            if l < L:
                down = np.diag(t_dn) @ (two_way * (eps[l].real / eps[l + 1].real) * (m / mu[l + 1]) * down)
    return out, per_layer


def solve_case(case, snowpack, emmodel_names=None):
    """The restatement on a fixture case; `snowpack`: the package's Snowpack built by build_snowpack (its interface and
    substrate objects are evaluated; its layers give frac_volume / liquid water of wet snow)."""
    wet = None
    if "volumetric_liquid_water" in case:
        wet = ([float(getattr(lay, "liquid_water", 0) or 0) for lay in snowpack.layers], [lay.frac_volume for lay in snowpack.layers])
    layers = O.make_layers(emmodel_names or case["emmodel"], case["frequency"], oracle_snowpack(case, wet))
    interfaces = [None if type(i).__name__ == "Flat" else i for i in snowpack.interfaces]
    sub, spec = snowpack.substrate, case.get("substrate")
    if spec and spec.get("substrate_model") == "flat":
        sub = ("flat", spec["permittivity_model"])
    elif spec and "reflector" in spec:
        sub = ("reflector", spec["reflector"]["V"], spec["reflector"]["H"])
    return first_order(layers, case["thickness"], case["frequency"], case["theta"], interfaces, sub), layers
