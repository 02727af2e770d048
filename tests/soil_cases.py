"""The inputs of the soil fixtures (tests/golden/make_soil_fixtures.py writes them, the soil tests read them): plain numbers,
no package imported, so that the generator builds them with the reference and the tests with smrt_amd."""
import numpy as np

# ---- (a) the three snow-on-soil cases of smrt/test/test_soil.py, with the constants that file asserts at 1e-4 -------------
WEGMULLER_SNOW = dict(thickness=[0.1, 0.1], density=[300, 300], temperature=[245, 245], radius=[200e-6, 400e-6],
                      stickiness=[1000, 1000], soil_temperature=270, roughness_rms=1e-2,
                      soil=dict(moisture=0.2, sand=0.4, clay=0.3, dry_matter=1100))
WEGMULLER_CASES = {   # permittivity model: (TbV, TbH)
    "soil_permittivity_dobson85_peplinski95": (262.5735899023818, 255.85856778263752),
    "soil_permittivity_dobson85_original": (262.56816517455616, 255.8528128244208),
    "soil_permittivity_montpetit08": (262.47365350048574, 255.75254543866822),
}

# ---- (b) soil_edge: the last layer has fewer streams than n_max_stream = 8, on both sides of 60 degrees -------------------
EDGE = dict(
    frequency=[19e9, 37e9], theta=[25.0, 55.0, 70.0],
    snow=[dict(thickness=[0.3, 0.5], density=[380.0, 220.0], temperature=[260.0, 265.0], corr_length=[1.0e-4, 2.0e-4]),
          dict(thickness=[0.2, 0.7], density=[400.0, 240.0], temperature=[255.0, 262.0], corr_length=[1.2e-4, 1.7e-4]),
          dict(thickness=[0.4, 0.4], density=[360.0, 200.0], temperature=[250.0, 258.0], corr_length=[0.8e-4, 2.2e-4])],
    substrates=[dict(model="soil_wegmuller", permittivity_model="soil_permittivity_dobson85_peplinski95", temperature=270.0,
                     soil=dict(moisture=0.2, sand=0.4, clay=0.3, dry_matter=1100.0), parameters=dict(roughness_rms=1e-2)),
                dict(model="soil_qnh", permittivity_model="soil_permittivity_dobson85_original", temperature=268.0,
                     soil=dict(moisture=0.15, sand=0.5, clay=0.2, dry_matter=1300.0), parameters=dict(H=0.3, Q=0.2, Nv=1.5, Nh=0.5)),
                dict(model="rough_choudhury79", permittivity_model="soil_permittivity_montpetit08", temperature=265.0,
                     soil={}, parameters=dict(roughness_rms=5e-5))])
EDGE_SO_OPTIONS = dict(n_iteration_max=6, relative_tolerance=0.0)   # every order is run: the orders compare one by one

# ---- (c) permittivities ---------------------------------------------------------------------------------------------------
SOIL_MODELS = {   # model: the attributes it reads
    "soil_permittivity_dobson85_peplinski95": ("temperature", "moisture", "sand", "clay"),
    "soil_permittivity_dobson85_original": ("temperature", "moisture", "sand", "clay"),
    "soil_permittivity_hut": ("temperature", "moisture", "sand", "clay", "dry_matter"),
    "soil_permittivity_montpetit08": ("temperature",),
}


def _points(t_lo, t_hi):
    rng = np.random.default_rng(1979)
    frequencies = [1.4e9, 6.9e9, 10.65e9, 18.7e9, 19e9, 23.8e9, 36.5e9, 37e9, 50e9, 89e9]
    return [dict(frequency=f, temperature=float(rng.uniform(t_lo, t_hi)), moisture=float(rng.uniform(0.05, 0.4)),
                 sand=float(rng.uniform(0.1, 0.7)), clay=float(rng.uniform(0.05, 0.3)), dry_matter=float(rng.uniform(900, 1500)))
            for f in frequencies]


PERMITTIVITY_POINTS = {"soil_permittivity_dobson85_peplinski95": _points(260.0, 295.0),
                       "soil_permittivity_dobson85_original": _points(260.0, 295.0),
                       "soil_permittivity_hut": _points(273.15, 300.0),          # thawed soil only
                       "soil_permittivity_montpetit08": _points(240.0, 273.15)}  # frozen soil only
BEDROCK_FREQUENCIES = [1.4e9, 37e9]


def last_layer_streams(eps_layers, n_max_stream):
    """Cosines of the streams of the last layer (smrt/rtsolver/streams.py:136-223): the Gauss-Legendre nodes are the streams of
    the most refringent layer, refracted into the last one; a stream that would be totally reflected does not exist there."""
    nodes, _ = np.polynomial.legendre.leggauss(2 * n_max_stream)
    mu_star = np.sort(nodes[nodes > 0])[::-1]
    e = np.asarray(eps_layers, complex)
    star = max(range(len(e)), key=lambda l: (e[l].real, e[l].imag, -l))
    sines = np.sqrt(e[star] / e[-1]).real * np.sqrt(1.0 - mu_star ** 2)
    return np.sqrt(1.0 - sines[sines < 1.0] ** 2)
