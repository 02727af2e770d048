"""NumPy restatement of the nadir LRM altimetry solver (smrt_amd/rtsolver/nadir_lrm_altimetry.py), written from the equations
(Lacroix et al. 2008 eq. 9; Brown 1977; Newkirk and Brown 1992; Larue et al. 2021), and the case table of the fixtures
tests/golden/nadir_lrm_altimetry_*.npz.  It stands in for the reference where the reference does not exist (the GPU tests);
tests/test_nadir_lrm_altimetry_cpu.py holds it to every fixture.

The vertical scattering distribution lives on the merge of two sorted sets of depths, the layer boundaries and the sub-gates
(regular in two-way travel time).  The merge is BY RANK, and the tie rule is stated here: AT EQUAL DEPTH A LAYER BOUNDARY
PRECEDES A GATE (z = 0 is always both).  On the merged grid: the two-way optical depth (prefix sum of 2 ke dz), the volume
backscatter of every interval integrated in closed form and attenuated from its top, the echo of every boundary attenuated
down to it; then the prefix sum of those and its differences between consecutive gates.  Only the first ngate x oversampling
sub-gates are made: a later one never reaches an output sample of the convolution.

Layer scalars come from the project's CPU oracle (oracle/dort_oracle.py); rough interfaces from the objects of the package the
snowpack was built with.
"""
import numpy as np
from scipy.special import erf, i0

from oracle import dort_oracle as O

C_SPEED = 299792458.0
EARTH_RADIUS = 6371000.0
REL_BAR = 1e-8          # every waveform sample against the peak of the case's total waveform
SMALL = dict(frequency=13.575e9, altitude=800e3, pulse_bandwidth=320e6, ngate=16, nominal_gate=5, beamwidth_alongtrack=1.29,
             beamwidth_acrosstrack=1.29)
_L3 = dict(thickness=[0.3, 0.9, 4.0], density=[280.0, 350.0, 420.0], temperature=[255.0, 258.0, 260.0],
           corr_length=[1.5e-4, 2.5e-4, 3e-4])
_IEM = dict(roughness_rms=5e-4, corr_length=1e-2)
_ROUGH = dict(interface=_IEM, substrate=dict(substrate_model="iem_fung92", permittivity_model=complex(5.0, 0.5), temperature=270.0,
                                             roughness_rms=5e-4, corr_length=1e-2))


def _many(n, d, seed):
    rng = np.random.RandomState(seed)
    return dict(thickness=[d] * n, density=list(rng.uniform(250.0, 450.0, n)), temperature=list(rng.uniform(250.0, 265.0, n)),
                corr_length=list(rng.uniform(1e-4, 3e-4, n)))


CASES = [
    dict(name="flat_L1", thickness=[5.0], density=[350.0], temperature=[260.0], corr_length=[3e-4]),
    dict(name="flat_L3", **_L3),
    dict(name="flat_L3_sigma", options=dict(theta_inc_sampling=1), sigma_surface=0.3, **_L3),
    dict(name="flat_L3_slope", options=dict(theta_inc_sampling=1), surface_slope=0.05, sigma_surface=0.1, **_L3),
    dict(name="flat_L3_pitchroll", options=dict(theta_inc_sampling=1), sensor=dict(SMALL, pitch_angle_deg=0.1, roll_angle_deg=0.05), **_L3),
    dict(name="flat_L3_contrib", options=dict(return_contributions=True, theta_inc_sampling=1), sigma_surface=0.2, **_L3),
    dict(name="rough_tis4", options=dict(theta_inc_sampling=4), **_ROUGH, **_L3),
    dict(name="rough_tis8_contrib", options=dict(theta_inc_sampling=8, return_contributions=True), **_ROUGH, **_L3),
    dict(name="rough_fast_coherent_sigma", options=dict(theta_inc_sampling=1, return_contributions=True), sigma_surface=0.3, **_ROUGH, **_L3),
    dict(name="rough_fast_coherent", options=dict(theta_inc_sampling=1), **_ROUGH, **_L3),
    dict(name="oversampled", options=dict(return_oversampled=True, theta_inc_sampling=1), **_ROUGH, **_L3),
    dict(name="os3_ng8", sensor=dict(SMALL, ngate=8, nominal_gate=3), options=dict(oversampling_time=3, theta_inc_sampling=1), **_ROUGH, **_L3),
    dict(name="os5_ng13", sensor=dict(SMALL, ngate=13, nominal_gate=4), options=dict(oversampling_time=5, theta_inc_sampling=1), **_ROUGH, **_L3),
    dict(name="L64", **_many(64, 0.05, 64)),
    dict(name="L65", **_many(65, 0.05, 65)),
    dict(name="thin_layers", **{k: v + w for (k, v), w in zip(_many(30, 0.004, 30).items(), ([3.0], [400.0], [260.0], [3e-4]))}),
    dict(name="shallow", thickness=[0.01], density=[300.0], temperature=[260.0], corr_length=[2e-4], options=dict(theta_inc_sampling=1), **_ROUGH),
    dict(name="deep", thickness=[2.0, 6.0, 12.0], density=[300.0, 380.0, 450.0], temperature=[255.0, 258.0, 260.0],
         corr_length=[2e-4, 3e-4, 3e-4]),
    dict(name="skip_pfs", options=dict(skip_pfs_convolution=True, theta_inc_sampling=1, return_contributions=True), **_ROUGH, **_L3),
    dict(name="nonscattering", emmodel="nonscattering", **_L3),
    dict(name="wet", volumetric_liquid_water=[0.02, 0.0, 0.0], **dict(_L3, temperature=[273.15, 258.0, 260.0])),
    dict(name="envisat_ku", sensor="envisat_ra2_Ku", thickness=[0.5, 2.0, 10.0], density=[300.0, 380.0, 450.0],
         temperature=[255.0, 258.0, 260.0], corr_length=[2e-4, 3e-4, 3e-4]),
]
DEFAULTS = dict(oversampling_time=10, return_oversampled=False, skip_pfs_convolution=False, return_contributions=False,
                compute_coherent_reflection=True, theta_inc_sampling=8)


def case_by_name(name):
    return next(c for c in CASES if c["name"] == name)


def solver_options(case):
    return dict(case.get("options", {}))


def make_sensor(case, api):
    s = case.get("sensor", SMALL)
    return api.lrm_altimeter_list.envisat_ra2("Ku") if s == "envisat_ra2_Ku" else api.lrm_altimeter_list.lrm_altimeter(channel="Ku", **s)


def build_snowpack(case, api):
    """The snowpack of a case with the constructors of `api` (the package under test or the reference)."""
    kw = {k: case[k] for k in ("temperature", "corr_length", "volumetric_liquid_water") if k in case}
    substrate = api.make_soil(**case["substrate"]) if "substrate" in case else None
    interface = [api.make_interface("iem_fung92", **case["interface"]) for _ in case["thickness"]] if "interface" in case else None
    sp = api.make_snowpack(case["thickness"], "exponential", density=case["density"], interface=interface, substrate=substrate, **kw)
    for name in ("sigma_surface", "surface_slope"):
        if name in case:
            setattr(sp, name, case[name])
    return sp


def oracle_layers(case, frequency, snowpack=None):
    sp = dict(thickness=np.asarray(case["thickness"], float), density=np.asarray(case["density"], float),
              temperature=np.asarray(case["temperature"], float), microstructure="exponential",
              corr_length=np.asarray(case["corr_length"], float))
    if "volumetric_liquid_water" in case:
        # the layers' own liquid_water (water / (ice + water) volume) and frac_volume (ice + water), as first_order_restatement.py
        sp["liquid_water"] = np.array([float(lay.liquid_water or 0) for lay in snowpack.layers])
        sp["frac_volume"] = np.array([float(lay.frac_volume) for lay in snowpack.layers])
    return O.make_layers(case.get("emmodel", "iba"), frequency, sp)


def layer_scalars(case, frequency, snowpack=None):
    """eps (real part), nadir extinction, backward scattering phase(-1, 1, pi)[0, 0] / 4 pi / eps of every layer."""
    layers = oracle_layers(case, frequency, snowpack)
    eps = np.array([lay.eps_eff.real for lay in layers])
    ke = np.array([lay.ks + lay.ka for lay in layers])
    bs = np.array([float(np.real(np.ravel(lay.phase(np.array([-1.0]), np.array([1.0]), np.pi, 2)[0, 0])[0])) if lay.ks > 0 else 0.0
                   for lay in layers]) / (4 * np.pi) / eps
    return eps, ke, bs, layers


def fresnel_power_v(eps_1, eps_2, mu):
    return O.flat_reflection(complex(eps_1), complex(eps_2), np.atleast_1d(np.asarray(mu, float)), 2)[0]


def boundary_numbers(case, sp, sensor, eps, mu_i, coherent):
    """(one-way transmission at nadir [L], echo [L + 1, n_mu]) of the boundaries: Flat ones from Fresnel with no echo, rough
    ones through the interface protocol plus the coherent part (Fung and Eom 1983 eq. 6)."""
    L, f = len(eps), float(sensor.frequency)
    above = np.concatenate([[1.0], eps[:-1]])
    k = 2 * np.pi * f / C_SPEED
    beta0 = np.sqrt(C_SPEED / (sensor.pulse_bandwidth * sensor.altitude)) * np.sqrt(2)
    beta12 = 1 / (k * sensor.altitude * beta0) ** 2 + beta0 ** 2 / 4
    trans, echo = np.empty(L), np.zeros((L + 1, len(mu_i)))

    def one(obj, e1, e2, substrate):
        mu = np.sqrt(1 - (1 - mu_i) / e1).real
        args = (f, e1) if substrate else (f, e1, e2)
        d = obj.diffuse_reflection_matrix(*args, mu, mu, np.pi, 2)
        d = np.asarray(getattr(d, "values", d), float)
        out = (np.diagonal(d[0, 0, 0]) if d.ndim == 5 else d[0]) / e1
        if coherent and hasattr(obj, "roughness_rms"):
            below = complex(obj.permittivity(f)) if substrate else e2
            out = out + fresnel_power_v(e1, below, mu) * np.exp(-4 * (k * obj.roughness_rms) ** 2 - (1 - mu ** 2) / beta12) / beta12 / (4 * np.pi)
        return out

    for l, itf in enumerate(sp.interfaces):
        if "interface" in case:
            t = itf.coherent_transmission_matrix(f, above[l], eps[l], np.ones(1), 2)
            trans[l] = np.asarray(getattr(t, "values", t), float)[0, 0]
            echo[l] = one(itf, above[l], eps[l], False)
        else:
            trans[l] = 1.0 - fresnel_power_v(above[l], eps[l], 1.0)[0]
    if sp.substrate is not None:
        echo[L] = one(sp.substrate, eps[-1], None, True)
    return trans, echo


def vertical_distribution(thickness, eps, ke, bs, trans, echo, step, n_sub, split):
    """The vertical scattering distribution on the first n_sub sub-gates (step: sub-gates per second).  Returns (rows, z_gate):
    rows [1, n_sub], or with `split` [2 n_mu + 1, n_sub]: surface rows, interface rows, volume; z_gate [n_sub], NaN where the
    snowpack has no gate."""
    L, n_mu = len(thickness), echo.shape[1]
    z_lay = np.concatenate([[0.0], np.cumsum(thickness)])
    t_lay = np.concatenate([[0.0], 2 * np.cumsum(thickness / (C_SPEED / np.sqrt(eps)))])
    ng = int(max(np.ceil(t_lay[-1] * step), 1))
    t_gate = np.arange(0, ng + 1) / step
    z_all = np.interp(t_gate, t_lay, z_lay)
    z_all[-1] += 0.01 * (z_all[-1] - z_all[-2])
    G = min(ng + 1, n_sub)
    z_gate = z_all[:G]
    # merge by rank; a boundary precedes a gate at equal depth
    nb = np.searchsorted(z_lay, z_gate, side="right")             # boundaries at or above every gate
    pos_gate = np.arange(G) + nb
    first_gate = np.searchsorted(nb, np.arange(L + 1), side="right")   # gates strictly above every boundary: first g with nb[g] > b
    kept = first_gate < G
    pos_bnd = (np.arange(L + 1) + first_gate)[kept]
    M = G + nb[-1]
    z = np.empty(M)
    z[pos_gate], z[pos_bnd] = z_gate, z_lay[kept]
    count = np.empty(M, int)                                      # boundaries at positions <= p
    count[pos_gate], count[pos_bnd] = nb, np.arange(1, L + 2)[kept]
    layer = np.minimum(count, L) - 1                              # the layer of the interval below point p
    cumtrans = np.concatenate([[1.0], np.cumprod(trans ** 2)])
    dtau = 2 * ke[layer[:-1]] * np.diff(z)
    tau = np.concatenate([[0.0], np.cumsum(dtau)])
    volume = np.zeros(M)
    volume[1:] = (1 - np.exp(-dtau)) / (2 * ke[layer[:-1]]) * bs[layer[:-1]] * (np.exp(-tau[:-1]) * cumtrans[np.minimum(count[:-1], L)])
    att_i = np.concatenate([[1.0], cumtrans[np.minimum(count[:-1], L)]])
    points = np.zeros((n_mu, M))
    points[:, pos_bnd] = echo[kept].T * (np.exp(-tau[pos_bnd]) * att_i[pos_bnd])

    def per_gate(v):
        c = np.cumsum(v, axis=-1)[..., pos_gate]
        out = np.zeros(v.shape[:-1] + (n_sub,))
        out[..., :G] = np.diff(np.concatenate([np.zeros(v.shape[:-1] + (1,)), c], axis=-1), axis=-1)
        return out

    zg = np.full(n_sub, np.nan)
    zg[:G] = z_gate
    if not split:
        return per_gate(points[0] + volume)[None], zg
    surface = np.zeros((n_mu, n_sub))
    surface[:, 0] = points[:, 0]
    points[:, 0] = 0.0
    return np.vstack([surface, per_gate(points), per_gate(volume)[None]]), zg


def pfs(sensor, gamma, otau, theta):
    e = C_SPEED / (sensor.altitude * (1 + sensor.altitude / EARTH_RADIUS)) * otau
    coef = sensor.antenna_gain ** 2 * sensor.wavelength ** 2 * C_SPEED / (4 * (4 * np.pi) ** 2 * sensor.altitude ** 3)
    negexp = lambda x: np.where(x <= 0, np.exp(np.minimum(x, 0)), 0)   # noqa: E731
    if theta == 0:
        return coef * negexp(-4 / gamma * e)
    return coef * negexp(-4 / gamma * (np.sin(theta) ** 2 + e * np.cos(2 * theta))) \
        * i0(4 / gamma * np.sqrt(np.maximum(e, 0)) * np.sin(2 * theta)) * (e >= 0)


def solve_case(case, api):
    """dict(waveform [rows, samples] (with contributions: surface, interfaces, volume, total), delay, gate, z_gate, eps, ke,
    backward_scattering, vertical)."""
    opt = dict(DEFAULTS, **solver_options(case))
    sensor, sp = make_sensor(case, api), build_snowpack(case, api)
    os_, nis, B = opt["oversampling_time"], opt["theta_inc_sampling"], sensor.pulse_bandwidth
    eps, ke, bs, _ = layer_scalars(case, float(sensor.frequency), sp)
    t_inc = np.linspace(0, sensor.ngate / B, nis + 1) if nis > 1 else np.zeros(1)
    mu_i = (1.0 / (1.0 + C_SPEED * t_inc / sensor.altitude) if nis > 1 else np.ones(1)) * np.cos(sensor.pitch_angle) * np.cos(sensor.roll_angle)
    trans, echo = boundary_numbers(case, sp, sensor, eps, mu_i, opt["compute_coherent_reflection"])
    N, step = sensor.ngate * os_, B * os_
    split = opt["return_contributions"] or nis > 1
    vertical, z_gate = vertical_distribution(np.asarray(case["thickness"], float), eps, ke, bs, trans, echo, step, N, split)
    t_gate = np.arange(N) / step
    t_nominal = sensor.nominal_gate / B
    gamma = 2 / 0.6931471805599453 * np.sin(np.deg2rad((sensor.beamwidth_alongtrack + sensor.beamwidth_acrosstrack) / 2) / 2) ** 2
    theta = sensor.off_nadir_angle + np.deg2rad(case.get("surface_slope", 0))
    convolve = lambda h, x: np.convolve(h, x)[:N]   # noqa: E731
    if opt["skip_pfs_convolution"]:
        w = vertical
    elif nis == 1:
        sigma_c = np.sqrt((0.513 / B) ** 2 + (2 * case.get("sigma_surface", 0) / C_SPEED) ** 2)
        shift = int((t_gate - t_nominal >= 0).argmax())
        h = pfs(sensor, gamma, t_gate[np.maximum(np.arange(N) - shift, 0)], theta)
        h = h * (1 + erf((t_gate - t_nominal) / (1.4142135623731 * sigma_c))) / 2 / B
        w = np.array([convolve(h, row) for row in vertical])
    else:
        n_mu = nis + 1
        h = pfs(sensor, gamma, t_gate - t_nominal, theta)
        interp = lambda f: np.interp(t_gate - t_nominal, t_inc, f, left=0)   # noqa: E731
        surface = interp(vertical[:n_mu, 0]) * h
        interfaces = np.zeros(N)
        for k in np.nonzero(vertical[n_mu] > 0)[0]:
            interfaces[k:] += (interp(vertical[n_mu:2 * n_mu, k]) * h)[:N - k]
        w = np.array([surface, interfaces, convolve(h, vertical[-1])]) / B
        if not opt["return_contributions"]:
            w = w.sum(axis=0)[None]
    if not opt["return_oversampled"] and os_ > 1:
        w = w.reshape(w.shape[0], -1, os_).mean(axis=-1)
        t_gate, z_gate = t_gate[::os_], z_gate[::os_]
    if opt["return_contributions"]:
        w = np.vstack([w, w.sum(axis=0)[None]])
    delay = t_gate - t_nominal
    return dict(waveform=w, delay=delay, gate=delay * B + sensor.nominal_gate, z_gate=z_gate, eps=eps, ke=ke, backward_scattering=bs,
                vertical=vertical)
