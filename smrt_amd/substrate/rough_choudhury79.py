"""Slightly rough boundary after Choudhury et al. 1979 (smrt/substrate/rough_choudhury79.py): both Fresnel reflectivities
times exp(-4 ksigma^2 mu^2), valid for ksigma << 1.  Where ksigma > 0.1 the reference raises; so does this class on the
host, and the device gives the pair the status SMRT_ERR_INPUT (an exception or NaN for that pair, by error_handling).
Passive mode; the device evaluates it per stream (csrc/dort_physics.hpp: soil_RvRh)."""
import numpy as np

from ..core.error import SMRTError
from .rough import AdjustedFresnelSubstrate, ksigma

KSIGMA_MAX = 0.1
OUT_OF_RANGE = "the Choudhury reflectivity is outside its validity range: ksigma must be <= 0.1 (ksigma << 1)"


class ChoudhuryReflectivity(AdjustedFresnelSubstrate):
    device_kind = "rough_choudhury79"
    args = ["roughness_rms"]

    def adjust(self, rv, rh, frequency, eps_1, mu1):
        ks = ksigma(frequency, eps_1, self.roughness_rms)
        if ks > KSIGMA_MAX:
            raise SMRTError(OUT_OF_RANGE)
        damping = np.exp(-4 * ks ** 2 * mu1 ** 2)
        return rv * damping, rh * damping

    def device_tail(self):
        return (float(self.roughness_rms), 0.0), (0.0, 0.0)
