"""Rough soil after Wegmuller & Maetzler 1999 (smrt/substrate/soil_wegmuller.py): R_h = Fresnel's times
exp(-ksigma^sqrt(0.1 mu)), R_v from R_h -- R_h mu^0.655 up to 60 degrees in the last layer, R_h (0.635 - 0.0014 (theta - 60))
beyond.  Passive mode; the device evaluates it per stream (csrc/dort_physics.hpp: soil_RvRh)."""
import numpy as np

from .rough import AdjustedFresnelSubstrate, ksigma


class SoilWegmuller(AdjustedFresnelSubstrate):
    device_kind = "soil_wegmuller"
    args = ["roughness_rms"]

    def adjust(self, rv, rh, frequency, eps_1, mu1):
        rh = rh * np.exp(-(ksigma(frequency, eps_1, self.roughness_rms) ** np.sqrt(0.1 * mu1)))
        beyond = mu1 < np.cos(60 * np.pi / 180)
        rv = np.where(beyond, rh * (0.635 - 0.0014 * (np.arccos(mu1) * 180 / np.pi - 60)), rh * mu1 ** 0.655)
        return rv, rh

    def device_tail(self):
        return (float(self.roughness_rms), 0.0), (0.0, 0.0)
