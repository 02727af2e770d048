"""Bedrock and subglacial-material permittivities on the host (the constants of smrt/permittivity/bedrock.py): a real part
and either a fixed imaginary part (Hartlieb et al. 2016, measured at 2.45 GHz) or a conductivity sigma in S/m, which gives
the imaginary part sigma / (2 pi f eps_0) (Tulaczyk & Foley 2020; Christianson et al. 2016).  One function
`bedrock_permittivity_<name>(frequency)` per material; none reads an attribute of the substrate."""
import numpy as np

from .soil import PERMITTIVITY_OF_FREE_SPACE, substrate_properties

_FIXED = {
    "granite_hartlieb16": 5.45 + 0.038j,
    "basalt_hartlieb16": 7.67 + 0.270j,
    "sandstone_hartlieb16": 7.67 + 0.081j,
}

_CONDUCTIVE = {   # real part, conductivity (S/m)
    "frozen_bedrock_tulaczyk20": (2.7, 0.0002),
    "saturated_bedrock_tulaczyk20": (9.5, 0.0055),
    "sandy_till_tulaczyk20": (13.0, 0.02),
    "fairbanks_silt_tulaczyk20": (24.0, 0.043),
    "clay_bearing_till_tulaczyk20": (13.0, 0.0575),
    "clay_tulaczyk20": (31.0, 0.24),
    "marine_clay_tulaczyk20": (31.0, 0.55),
    "debris_laden_ice_christianson16": (3.1, 8.0e-5),
    "sand_christianson16": (2.6, 1.3e-4),
    "groundwater_till_christianson16": (36.0, 0.037),
    "freshwater_till_christianson16": (13.0, 2.5e-4),
    "frozen_till_christianson16": (2.9, 3.4e-4),
    "frozen_bedrock_christianson16": (2.7, 2.0e-4),
    "unfrozen_bedrock_christianson16": (12.0, 0.0048),
}

BEDROCK_MODELS = []


def _define(name, function):
    function.__name__ = function.__qualname__ = "bedrock_permittivity_" + name
    globals()[function.__name__] = substrate_properties()(function)
    BEDROCK_MODELS.append(function.__name__)


for _name, _value in _FIXED.items():
    _define(_name, lambda frequency, _v=_value: _v)
for _name, (_real, _sigma) in _CONDUCTIVE.items():
    _define(_name, lambda frequency, _r=_real, _s=_sigma: _r + 1j * (_s / (2 * np.pi * frequency * PERMITTIVITY_OF_FREE_SPACE)))
