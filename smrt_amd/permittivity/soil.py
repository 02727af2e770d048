"""Soil dielectric models on the host, restated from the equations of smrt/permittivity/soil.py and vectorised: every
argument besides the frequency may be an array (one element per snowpack of a device batch), the result has one complex
value per element.  The substrate classes call them with the attributes named in `required_arguments`
(core/substrate.py); a batch evaluates a model once per frequency on the columns of its snowpacks.

  soil_permittivity_dobson85_peplinski95   Dobson et al. 1985 with the conductivity fit of Peplinski et al. 1995
  soil_permittivity_dobson85_original      Dobson et al. 1985 with its own conductivity (eq. 8 of Peplinski et al. 1995)
  soil_permittivity_hut                    Pulliainen et al. 1999 / Lemmetyinen et al. 2010, thawed soil only
  soil_permittivity_montpetit08            Montpetit et al. 2018, frozen soil only: three values, linear in the frequency
"""
import numpy as np

from ..core.error import SMRTError
from ..core.globalconstants import C_SPEED

PERMITTIVITY_OF_FREE_SPACE = 1 / (4e-7 * np.pi * C_SPEED ** 2)


def substrate_properties(*required):
    """Names the attributes of the substrate a permittivity function is called with, after the frequency."""
    def decorate(function):
        function.required_arguments = list(required)
        function.optional_arguments = {}
        return function
    return decorate


def _dobson85(frequency, temperature, moisture, sand, clay, sigma_eff):
    e_w_inf, e_s, rho_b, rho_s = 4.9, 4.7, 1.3, 2.664
    temp = np.asarray(temperature, float) - 273.15
    moisture = np.asarray(moisture, float)
    beta_prime = 1.2748 - 0.519 * sand - 0.152 * clay          # Dobson et al. 1985, eq. 30
    beta_second = 1.33797 - 0.603 * sand - 0.166 * clay        # eq. 31
    # static permittivity and relaxation time of water (Stogryn 1971)
    e_w0 = 87.134 - 1.949e-1 * temp - 1.276e-2 * temp ** 2 + 2.491e-4 * temp ** 3
    rt_w = (1.1109e-10 - 3.824e-12 * temp + 6.938e-14 * temp ** 2 - 5.096e-16 * temp ** 3) / (2 * np.pi)
    e_fw_prime = e_w_inf + (e_w0 - e_w_inf) / (1 + (2 * np.pi * frequency * rt_w) ** 2)
    e_fw_second = 2 * np.pi * frequency * rt_w * (e_w0 - e_w_inf) / (1 + (2 * np.pi * frequency * rt_w) ** 2) \
        + sigma_eff * (rho_s - rho_b) / (2 * np.pi * frequency * PERMITTIVITY_OF_FREE_SPACE * rho_s * moisture)
    real = (1 + (rho_b / rho_s) * (e_s ** 0.65 - 1) + moisture ** beta_prime * e_fw_prime ** 0.65 - moisture) ** (1 / 0.65)
    imag = (moisture ** beta_second * e_fw_second ** 0.65) ** (1 / 0.65)
    return real + 1j * imag


@substrate_properties("temperature", "moisture", "sand", "clay")
def soil_permittivity_dobson85_peplinski95(frequency, temperature, moisture, sand, clay):
    sand, clay = np.asarray(sand, float), np.asarray(clay, float)
    sigma_eff = 0.0467 + 0.2204 * 1.3 - 0.4111 * sand + 0.6614 * clay      # Peplinski et al. 1995, eq. 10
    return _dobson85(frequency, temperature, moisture, sand, clay, sigma_eff)


@substrate_properties("temperature", "moisture", "sand", "clay")
def soil_permittivity_dobson85_original(frequency, temperature, moisture, sand, clay):
    sand, clay = np.asarray(sand, float), np.asarray(clay, float)
    sigma_eff = -1.645 + 1.939 * 1.3 - 2.25622 * sand + 1.594 * clay       # Peplinski et al. 1995, eq. 8
    return _dobson85(frequency, temperature, moisture, sand, clay, sigma_eff)


@substrate_properties("temperature", "moisture", "sand", "clay")
def soil_permittivity_dobson85(frequency, temperature, moisture, sand, clay):
    raise SMRTError("the soil permittivity model 'dobson85' is outside the scope of smrt_amd, as the reference refuses it: "
                    "what it used to name is 'soil_permittivity_dobson85_peplinski95', and the model of Dobson et al. (1985) "
                    "itself is 'soil_permittivity_dobson85_original'")


@substrate_properties("temperature", "moisture", "sand", "clay", "dry_matter")
def soil_permittivity_hut(frequency, temperature, moisture, sand, clay, dry_matter):
    ew_inf = 4.9
    temp = np.asarray(temperature, float) - 273.15
    if np.any(temp < 0):
        raise SMRTError("soil_permittivity_hut requires above freezing point temperatures")
    ew0 = 87.74 - 0.40008 * temp + 9.398e-4 * temp ** 2 + 1.410e-6 * temp ** 3
    tw = 1 / (2 * np.pi) * (1.1109e-10 - 3.824e-12 * temp + 6.938e-14 * temp ** 2 - 5.096e-16 * temp ** 3)
    ew_r = ew_inf + (ew0 - ew_inf) / (1 + (2 * np.pi * frequency * tw) ** 2)
    ew_i = (ew0 - ew_inf) * 2 * np.pi * frequency * tw / (1 + (2 * np.pi * frequency * tw) ** 2)
    beta = 1.09 - 0.11 * np.asarray(sand, float) + 0.18 * np.asarray(clay, float)
    epsalf = 1 + 0.65 * np.asarray(dry_matter, float) / 1000.0 + np.asarray(moisture, float) ** beta * ((ew_r + 1j * ew_i) ** 0.65 - 1)
    return epsalf ** (1 / 0.65)


_MONTPETIT_F = np.array([10.65e9, 19e9, 37e9])
_MONTPETIT_EPS = np.array([complex(3.18, 0.0061), complex(3.42, 0.0051), complex(4.47, 0.33)])


@substrate_properties("temperature")
def soil_permittivity_montpetit08(frequency, temperature):
    temperature = np.asarray(temperature, float)
    if np.any(temperature > 273.15):
        raise SMRTError("soil_permittivity_monpetit is not implemented for above freezing temperatures.")
    # linear between the two neighbours, the outer segments continued beyond the table
    hi = int(np.clip(np.searchsorted(_MONTPETIT_F, frequency), 1, len(_MONTPETIT_F) - 1))
    lo = hi - 1
    slope = (_MONTPETIT_EPS[hi] - _MONTPETIT_EPS[lo]) / (_MONTPETIT_F[hi] - _MONTPETIT_F[lo])
    return np.zeros(temperature.shape) + (slope * (frequency - _MONTPETIT_F[lo]) + _MONTPETIT_EPS[lo])
