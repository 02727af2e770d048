"""NumPy restatement of the successive-order-of-scattering solution in ACTIVE mode (backscatter order by order), written
from the equations (Lenoble et al. 2007, eq. 66; Greenwald et al. 2005, eq. 2, with the incident beams as columns), and the
case table of the fixtures tests/golden/successive_order_active_*.npz.  It stands in for the reference where the reference
does not exist (the GPU tests); tests/test_successive_order_active_cpu.py holds it to every fixture.

Three polarisations (V, H, U) everywhere.  Direction index inside a layer of n streams: d < 3 n upward (stream d // 3,
polarisation d % 3), 3 n <= d < 6 n downward.  Column c = (incident stream jj, incident polarisation p) = jj * npol_inc + p.
Passes: one coherent pass (no phase matrix, never stops) and one per azimuth mode; from every mode's orders (1 + [m > 0]) x the
coherent pass's orders are subtracted, for ALL orders, also those after the mode stopped (they then hold minus the coherent
remainder, as in the reference).

Layer scalars, phase matrices, streams, Fresnel coefficients and the interpolation to the sensor's angles come from the
project's CPU oracle (oracle/dort_oracle.py).
"""
import numpy as np

from oracle import dort_oracle as O

PARITY_RTOL = 1e-8   # x the largest co-polarised total: the project's active-mode bar (profiles/first_order_parity.txt)

_SOIL = dict(thickness=[0.2, 0.5], density=[250.0, 350.0], temperature=[255.0, 262.0], corr_length=[2e-4, 4e-4],
             substrate=dict(substrate_model="flat", permittivity_model=complex(5.0, 0.5), temperature=265.0))
_EXP = dict(emmodel="iba", microstructure_model="exponential")
CASES = [
    dict(name="iba_L1_n4", frequency=13e9, theta=[40.0], thickness=[1.0], density=[300.0], temperature=[260.0],
         corr_length=[3e-4], n_max_stream=4, n_iteration_max=6, **_EXP),
    dict(name="iba_refraction_L3_n6", frequency=13e9, theta=[25.0, 45.0], thickness=[0.3, 0.2, 2.0], density=[200.0, 450.0, 300.0],
         temperature=[250.0, 255.0, 260.0], corr_length=[1e-4, 5e-5, 1e-4], n_max_stream=6, n_iteration_max=10, **_EXP),
    dict(name="iba_deep_L2_n8", frequency=37e9, theta=[40.0], thickness=[0.05, 3.0], density=[300.0, 350.0],
         temperature=[255.0, 262.0], corr_length=[1e-4, 4e-4], n_max_stream=8, n_iteration_max=6, **_EXP),
    dict(name="iba_soil_L2_n8", frequency=13e9, theta=[30.0, 50.0], n_max_stream=8, n_iteration_max=8, **_SOIL, **_EXP),
    dict(name="iba_soil_L2_n8_V", frequency=13e9, theta=[30.0], n_max_stream=8, n_iteration_max=4, incident_polarizations="V",
         **_SOIL, **_EXP),
    dict(name="iba_soil_L2_n8_VHU", frequency=13e9, theta=[30.0], n_max_stream=8, n_iteration_max=4, incident_polarizations="VHU",
         **_SOIL, **_EXP),
    dict(name="iba_soil_L2_n16_m0", frequency=13e9, theta=[30.0, 50.0], n_max_stream=16, n_iteration_max=4, m_max=0, **_SOIL, **_EXP),
    dict(name="dmrt_L10_n32", emmodel="dmrt_qca_shortrange", microstructure_model="sticky_hard_spheres", frequency=13e9, theta=[35.0],
         thickness=[0.1] * 10, density=list(np.linspace(200.0, 380.0, 10)), temperature=list(np.linspace(250.0, 265.0, 10)),
         radius=list(np.linspace(2e-4, 5e-4, 10)), stickiness=[0.2] * 10, n_max_stream=32, n_iteration_max=8),
    dict(name="tol0_n8", frequency=13e9, theta=[30.0, 50.0], n_max_stream=8, n_iteration_max=6, relative_tolerance=0.0, **_SOIL, **_EXP),
]
OPTION_KEYS = ("n_max_stream", "n_iteration_max", "relative_tolerance", "m_max", "incident_polarizations")


def case_by_name(name):
    return next(c for c in CASES if c["name"] == name)


def solver_options(case):
    return {k: case[k] for k in OPTION_KEYS if k in case}


def build_snowpack(case, api):
    """The snowpack of a case with the constructors of `api` (the package under test or the reference)."""
    kw = {k: case[k] for k in ("temperature", "corr_length", "radius", "stickiness") if k in case}
    sub = case.get("substrate")
    substrate = api.make_soil(**sub) if sub else None
    return api.make_snowpack(case["thickness"], case["microstructure_model"], density=case["density"], substrate=substrate, **kw)


def oracle_snowpack(case):
    sp = dict(thickness=np.asarray(case["thickness"], float), density=np.asarray(case["density"], float),
              temperature=np.asarray(case["temperature"], float), microstructure=case["microstructure_model"])
    for k in ("corr_length", "radius", "stickiness"):
        if k in case:
            sp[k] = np.asarray(case[k], float)
    return sp


def oracle_substrate(case):
    sub = case.get("substrate")
    return dict(kind="flat", eps=complex(sub["permittivity_model"])) if sub else None


# ---- pieces the tests hold on their own --------------------------------------------------------------------------------
def incident_streams(outmu, theta_inc_deg):
    """The one or two air streams that bracket each cos(theta_inc), as a sorted list (prepare_incident_streams); outmu is
    descending."""
    outmu = np.asarray(outmu, float)
    inc = set()
    for mi in np.cos(np.deg2rad(np.atleast_1d(np.asarray(theta_inc_deg, float)))):
        i0 = int(np.searchsorted(-outmu, -mi))
        if i0 == 0:
            inc.add(0)
        elif i0 == len(outmu):
            inc.add(i0 - 1)
        else:
            inc.update((i0, i0 - 1))
    return sorted(inc)


def pass_tolerance(mode, relative_tolerance, own_largest_order0):
    """The tolerance a mode pass forms by itself from its own order 0.  At order 0 the profile is zero, so the emerging
    radiance is the specular reflection of the pass's own incident columns; those of a mode m >= 1 are twice mode 0's (a
    scaling by 2 is exact in binary floating point), so halving gives mode 0's largest radiance bit for bit."""
    return relative_tolerance * (own_largest_order0 / (2.0 if mode > 0 else 1.0))


def _flat3(d):
    """[3, n] -> stream-major, polarisation fastest."""
    return np.asarray(d, float).T.reshape(-1)


# ---- the solution ----------------------------------------------------------------------------------------------------
def successive_order_backscatter(layers, thickness, theta_inc_deg, n_max_stream=32, n_iteration_max=50, relative_tolerance=0.001,
                                 m_max=2, incident_polarizations="VH", substrate=None, phi=np.pi):
    """Oracle layers (eps_eff, ks, ka, ft_even_phase) -> dict(sigma [3, 3, n_theta_inc, n_iteration_max + 1] (intensity ratio;
    first index the scattered, second the incident polarisation), pass_max: per pass (coherent first, then the modes) the
    largest emerging radiance of every order run, sublayers, streams, incident (the incident streams), tolerance)."""
    L, NO = len(layers), n_iteration_max
    eps = [complex(lay.eps_eff) for lay in layers]
    st = O.compute_streams(n_max_stream, eps)
    itf = O.interface_diagonals(eps, st, 3, substrate=substrate)
    K, ext, n = [], [], []
    W = [[] for _ in range(m_max + 1)]
    for l, lay in enumerate(layers):
        ke = lay.ks + lay.ka
        mu, w = st.mu[l], st.weight[l]
        K.append(max(int(np.ceil(ke * thickness[l] / 0.1)), 1))
        n.append(3 * len(mu))
        full = np.concatenate((mu, -mu))
        P = np.asarray(lay.ft_even_phase(full, full, m_max, 3), float)
        for m in range(m_max + 1):
            W[m].append((1.0 / ke) * ((0.5 if m == 0 else 0.25) * O.compress(P[:, :, m])) * np.tile(np.repeat(w, 3), 2)[None, :])
        ext.append(np.exp(-(ke * thickness[l]) / K[l] / np.repeat(mu, 3))[:, None])
    Rtop, Ttop = [_flat3(x)[:, None] for x in itf["Rtop"]], [_flat3(x)[:, None] for x in itf["Ttop"]]
    Rbot, Tbot = [_flat3(x)[:, None] for x in itf["Rbot"]], [_flat3(x)[:, None] for x in itf["Tbot"]]
    Rair, Tair = _flat3(itf["Rbot_air"])[:, None], _flat3(itf["Tbot_air"])[:, None]
    inc = incident_streams(st.outmu, theta_inc_deg)
    npi = len(incident_polarizations)
    C, n_out = npi * len(inc), 3 * st.n_air
    incident0 = np.zeros((n_out, C))
    for jj, i in enumerate(inc):
        for p in range(npi):
            incident0[3 * i + p, jj * npi + p] = 1.0 / (2 * np.pi * st.outweight[i])

    state = dict(tolerance=0.0)

    def run_pass(Wm, incident, may_stop):
        previous = [np.zeros((K[l] + 1, 2 * n[l], C)) for l in range(L)]
        emerging_orders = np.zeros((n_out, C, NO))
        largest_orders = []
        for order in range(NO):
            new = [np.zeros_like(p) for p in previous]
            S = []
            for l in range(L):
                mean = (previous[l][:-1] + previous[l][1:]) / 2
                S.append(np.zeros_like(mean) if Wm is None else np.einsum("dq,kqc->kdc", Wm[l], mean))
            carry = Tair * incident if order == 0 else np.zeros((0, C))
            for l in range(L):                                                   # downwards
                nl = n[l]
                I = Rtop[l] * previous[l][0, :nl]
                m = min(nl, len(carry))
                I[:m] += carry[:m]
                new[l][0, nl:] = I
                for k in range(K[l]):
                    I = I * ext[l] + S[l][k, nl:] * (1 - ext[l])
                    new[l][k + 1, nl:] = I
                carry = Tbot[l] * I
            carry = np.zeros((0, C))
            for l in range(L - 1, -1, -1):                                       # upwards
                nl = n[l]
                I = Rbot[l] * previous[l][-1, nl:]
                m = min(nl, len(carry))
                I[:m] += carry[:m]
                new[l][-1, :nl] = I
                for k in range(K[l] - 1, -1, -1):
                    I = I * ext[l] + S[l][k, :nl] * (1 - ext[l])
                    new[l][k, :nl] = I
                carry = Ttop[l] * I
            emerging = carry[:n_out].copy()
            if order == 0:
                emerging += Rair * incident
            emerging_orders[:, :, order] = emerging
            previous = new
            largest = float(np.max(emerging))
            largest_orders.append(largest)
            if state["tolerance"] == 0:
                state["tolerance"] = relative_tolerance * largest
            if may_stop and largest < state["tolerance"]:
                break
        return emerging_orders, largest_orders

    coherent, coherent_max = run_pass(None, incident0, False)
    state["tolerance"] = 0.0
    pass_max = [coherent_max]
    total = np.zeros((3, st.n_air, npi, len(inc), NO))
    for m in range(m_max + 1):
        factor = 1.0 + float(m > 0)
        Im, largest = run_pass(W[m], factor * incident0, True)
        pass_max.append(largest)
        Im = Im - coherent * factor
        Im = Im.reshape(st.n_air, 3, len(inc), npi, NO).transpose(1, 0, 3, 2, 4)
        if m == 0:
            total[0:2, :, 0:2] += Im[0:2, :, 0:2]
        else:
            total[0:2] += Im[0:2] * np.cos(m * phi)
            total[2:] += Im[2:] * np.sin(m * phi)
    back = np.zeros((3, 3, len(inc), NO))
    for j, i in enumerate(inc):
        back[:, :npi, j] = total[:, i, :, j]
    back = np.append(back, np.sum(back, axis=-1)[..., None], axis=-1)
    user_mu = np.cos(np.deg2rad(np.atleast_1d(np.asarray(theta_inc_deg, float))))
    outmu = st.outmu[inc]
    sigma = np.stack([O.interpolate_active(outmu, back[..., k], user_mu) for k in range(NO + 1)], axis=-1)
    return dict(sigma=sigma, pass_max=pass_max, sublayers=np.array(K), streams=np.array([len(mu) for mu in st.mu]),
                incident=np.array(inc), outmu=st.outmu, tolerance=state["tolerance"], columns=C)


def solve_case(case, **overrides):
    """The restatement on a case of the table; returns (solution dict, oracle layers)."""
    layers = O.make_layers(case["emmodel"], case["frequency"], oracle_snowpack(case))
    opts = dict(solver_options(case), **overrides)
    return successive_order_backscatter(layers, case["thickness"], case["theta"], substrate=oracle_substrate(case), **opts), layers


def parity_bar(sigma):
    """1e-8 x the largest co-polarised total."""
    return PARITY_RTOL * max(float(np.max(np.abs(sigma[0, 0, :, -1]))), float(np.max(np.abs(sigma[1, 1, :, -1]))))
