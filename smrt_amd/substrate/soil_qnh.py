"""Rough soil after Wang 1983, the QNH model (smrt/substrate/soil_qnh.py): the two Fresnel reflectivities are mixed by Q, then
damped by exp(-H mu^N), with one exponent per polarisation (Nv, Nh; each defaults to N).  Passive mode; the device
evaluates it per stream (csrc/dort_physics.hpp: soil_RvRh).  Unlike the reference's, a call leaves the object as it was:
Nv and Nh stay NaN when they were not given."""
import numpy as np

from .rough import AdjustedFresnelSubstrate


class SoilQNH(AdjustedFresnelSubstrate):
    device_kind = "soil_qnh"
    args = ["H"]
    optional_args = {"Q": 0.0, "N": 0.0, "Nv": np.nan, "Nh": np.nan}

    def exponents(self):
        return (self.N if np.isnan(self.Nv) else self.Nv), (self.N if np.isnan(self.Nh) else self.Nh)

    def adjust(self, rv, rh, frequency, eps_1, mu1):
        nv, nh = self.exponents()
        mixed_v = ((1 - self.Q) * rv + self.Q * rh) * np.exp(-self.H * (mu1 ** nv))
        mixed_h = ((1 - self.Q) * rh + self.Q * rv) * np.exp(-self.H * (mu1 ** nh))
        return mixed_v, mixed_h

    def device_tail(self):
        nv, nh = self.exponents()
        return (float(self.H), float(self.Q)), (float(nv), float(nh))
