"""NumPy restatement of the multi-Fresnel thermal emission solution, written from the equations (Hebert et al. 2015; annex of
Zeiger et al. 2024; rigorous Fresnel coefficients of Maezawa & Miyauchi 2009), and the case table of the fixtures
tests/golden/multifresnel_*.npz.  It stands in for the reference where the reference does not exist (the GPU tests);
tests/test_multifresnel_cpu.py holds it to every fixture.

Per sensor angle, from mu = cos(theta) in the air, for every layer from the top down: power reflectivities r_V, r_H of the
interface above the layer and the refracted cosine mu2; tau = 2 Im sqrt(eps2) k0 d / mu2 clipped to [0, what the angle has
left]; t = exp(-tau); the 2 x 3 matrix (third row 0 0 1 implicit)

    [ 1/t   -r t        l13 - r l23          ]                l13 = -(1/t - 1) T
    [ r/t   (1 - 2r) t  r l13 + (1 - 2r) l23 ] / (1 - r)      l23 = (1 - t) T

multiplied into the running product from the right; Tb = -M10 M02 / M00 + M12.

Two facts about the pruning rule, both reproduced here and on the device, both found while the fixtures were made:
  * the chain stops after the first layer at which the steepest angle's remainder is NEGATIVE.  The remainder is
    x - min(max(tau, 0), x): never negative in IEEE arithmetic.  The stop never fires: an exhausted angle keeps every
    interface below with t = 1, the steepest one included, and layers_used is always the number of layers.
  * prune_deep_snowpack=None makes the reference clip against NaN: every Tb is NaN.  Here None means no clipping, which is what
    the reference computes for prune_deep_snowpack=inf; the fixture of `firn_noprune` is the reference at inf.

Layer scalars come from the project's CPU oracle (oracle/dort_oracle.py).
"""
import numpy as np

from oracle import dort_oracle as O

TB_ATOL = 1e-6   # kelvin: the project's bar for a brightness temperature against the reference
C_SPEED = 299792458.0
SUBSTRATE_DEPTH = 1e10

_FIRN = dict(frequency=19e9, theta=[0.0, 20.0, 40.0, 55.0, 70.0], n_layers=300, layer_thickness=0.05, seed=20261017)
_SOIL = dict(substrate_model="flat", permittivity_model=complex(5.0, 0.5), temperature=270.0)
CASES = [
    dict(name="L1", emmodel="nonscattering", frequency=1.4e9, theta=[0.0, 40.0], thickness=[10.0], density=[350.0], temperature=[250.0]),
    dict(name="soil_L3", emmodel="nonscattering", frequency=1.4e9, theta=[10.0, 50.0], thickness=[0.3, 0.7, 2.0],
         density=[250.0, 380.0, 450.0], temperature=[255.0, 260.0, 265.0], substrate=_SOIL),
    dict(name="firn_L300_19GHz", emmodel="nonscattering", **_FIRN),
    dict(name="firn_prune1", emmodel="nonscattering", prune_deep_snowpack=1, **_FIRN),
    dict(name="firn_noprune", emmodel="nonscattering", prune_deep_snowpack=None, **_FIRN),
    dict(name="iba_L4", emmodel="iba", frequency=19e9, theta=[30.0, 55.0], thickness=[0.2, 0.5, 1.0, 30.0],
         density=[220.0, 300.0, 360.0, 420.0], temperature=[250.0, 255.0, 258.0, 260.0], corr_length=[1e-4, 2e-4, 2.5e-4, 3e-4]),
    dict(name="firn_L4000", emmodel="nonscattering", frequency=1.4e9, theta=[0.0, 40.0, 55.0], n_layers=4000, layer_thickness=0.05,
         seed=20261018),
    dict(name="soil_lossless", emmodel="nonscattering", frequency=1.4e9, theta=[10.0, 50.0], thickness=[0.3, 0.7, 2.0],
         density=[250.0, 380.0, 450.0], temperature=[255.0, 260.0, 265.0],
         substrate=dict(substrate_model="flat", permittivity_model=complex(5.0, 1e-9), temperature=270.0)),
]
PRUNE_DEFAULT = 10


def case_by_name(name):
    return next(c for c in CASES if c["name"] == name)


def solver_options(case):
    return {"prune_deep_snowpack": case["prune_deep_snowpack"]} if "prune_deep_snowpack" in case else {}


def profile(case):
    """dict(thickness, density, temperature, corr_length) of a case as lists; the firn profiles are generated from the seed:
    density rising with depth towards 800 kg/m3 with layer-to-layer noise, temperature relaxing to 245 K under a 10 m wave."""
    if "thickness" in case:
        L = len(case["thickness"])
        return dict(thickness=list(case["thickness"]), density=list(case["density"]), temperature=list(case["temperature"]),
                    corr_length=list(case.get("corr_length", [1e-4] * L)))
    rng = np.random.RandomState(case["seed"])
    L, d = case["n_layers"], case["layer_thickness"]
    z = (np.arange(L) + 0.5) * d
    density = 350.0 + 450.0 * (1.0 - np.exp(-z / 60.0)) + rng.uniform(-30.0, 30.0, L)
    temperature = 245.0 + 12.0 * np.exp(-z / 3.0) * np.cos(z / 3.0) + rng.uniform(-0.2, 0.2, L)
    return dict(thickness=[d] * L, density=list(density), temperature=list(temperature), corr_length=[1e-4] * L)


def build_snowpack(case, api):
    """The snowpack of a case with the constructors of `api` (the package under test or the reference: make_snowpack,
    make_soil)."""
    p = profile(case)
    substrate = api.make_soil(**case["substrate"]) if "substrate" in case else None
    return api.make_snowpack(p["thickness"], "exponential", density=p["density"], temperature=p["temperature"],
                             corr_length=p["corr_length"], substrate=substrate)


def oracle_layers(case, frequency=None, emmodel=None):
    p = profile(case)
    sp = dict(thickness=np.asarray(p["thickness"]), density=np.asarray(p["density"]), temperature=np.asarray(p["temperature"]),
              microstructure="exponential", corr_length=np.asarray(p["corr_length"]))
    return O.make_layers(emmodel or case["emmodel"], frequency or case["frequency"], sp)


# ---- the solution ----------------------------------------------------------------------------------------------------
def fresnel_power(eps1, eps2, mu):
    """r [2 (V, H), n_angles] and the refracted cosines for the cosines `mu` in medium 1."""
    eps1, eps2 = complex(eps1), complex(eps2)
    n1 = np.sqrt(eps1)
    kz2 = n1.real ** 2 * (1.0 - mu ** 2)
    kyi = -np.sqrt(eps1 - kz2 + 0j)
    kyt = -np.sqrt(eps2 - kz2 + 0j)
    rh = (kyi - kyt) / (kyi.conjugate() + kyt)
    rv = n1.conjugate() * (eps2 * kyi - eps1 * kyt) / (n1 * (eps2 * kyi.conjugate() + eps1.conjugate() * kyt))
    return np.stack((rv.real ** 2 + rv.imag ** 2, rh.real ** 2 + rh.imag ** 2)), -kyt.real / np.sqrt(eps2).real


def multifresnel(eps, temperature, thickness, frequency, theta_deg, prune_deep_snowpack=PRUNE_DEFAULT):
    """eps, temperature, thickness: per layer, the substrate already appended.  Returns dict(tb [n_theta, 2], layers_used,
    tau_snowpack, first_clipped [n_theta] (-1: never), remainders (the steepest angle's, after every layer used))."""
    mu = np.cos(np.deg2rad(np.asarray(theta_deg, float)))
    steepest = int(np.argmax(mu))
    left = np.full(len(mu), np.inf if prune_deep_snowpack is None else float(prune_deep_snowpack))
    k0 = 2 * np.pi * frequency / C_SPEED
    eps1, M = 1.0, None
    tau_snowpack, used, remainders = 0.0, 0, []
    first_clipped = np.full(len(mu), -1)
    with np.errstate(all="ignore"):
        for l, (eps2, T, d) in enumerate(zip(eps, temperature, thickness)):
            r, mu2 = fresnel_power(eps1, eps2, mu)
            raw = 2 * np.sqrt(complex(eps2)).imag * (k0 * d) / mu2
            tau = np.minimum(np.maximum(raw, 0.0), left)
            first_clipped[(first_clipped < 0) & (tau < raw)] = l
            t = np.exp(-tau)[None, :]
            l13, l23 = -(1 / t - 1) * T, (1 - t) * T
            Lm = np.empty((2, 3, 2, len(mu)))
            Lm[0, 0], Lm[0, 1], Lm[0, 2] = 1 / t, -r * t, l13 - r * l23
            Lm[1, 0], Lm[1, 1], Lm[1, 2] = r / t, (1 - 2 * r) * t, r * l13 + (1 - 2 * r) * l23
            Lm /= 1 - r
            if M is None:
                M = Lm
            else:
                P = np.empty_like(M)
                P[0] = M[0, 0] * Lm[0] + M[0, 1] * Lm[1]
                P[1] = M[1, 0] * Lm[0] + M[1, 1] * Lm[1]
                P[:, 2] += M[:, 2]
                M = P
            left = left - tau
            tau_snowpack += tau[steepest]
            remainders.append(left[steepest])
            used = l + 1
            if left[steepest] < 0:
                break
            mu, eps1 = mu2, eps2
        tb = -M[1, 0] * M[0, 2] / M[0, 0] + M[1, 2]
    return dict(tb=np.ascontiguousarray(tb.T), layers_used=used, tau_snowpack=float(tau_snowpack), first_clipped=first_clipped,
                remainders=np.array(remainders), m00=float(np.abs(M[0, 0]).max()))


def solve_case(case, emmodel=None):
    """(solution, layers) of a case through the restatement."""
    layers = oracle_layers(case, emmodel=emmodel)
    p = profile(case)
    eps = [lay.eps_eff for lay in layers]
    temperature, thickness = list(p["temperature"]), list(p["thickness"])
    if "substrate" in case:
        eps.append(case["substrate"]["permittivity_model"])
        temperature.append(case["substrate"]["temperature"])
        thickness.append(SUBSTRATE_DEPTH)
    sol = multifresnel(eps, temperature, thickness, case["frequency"], case["theta"], case.get("prune_deep_snowpack", PRUNE_DEFAULT))
    return sol, layers
