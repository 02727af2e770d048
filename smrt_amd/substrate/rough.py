"""Substrates made of a rough-interface model (the role of smrt/core/interface.py:169-240, substrate_from_interface): the
medium below is the substrate's own permittivity, the methods are the substrate protocol the DORT solver evaluates on
the streams of the last layer (rtsolver/dort.py:substrate_matrices, _substrates_on_host) -- specular_reflection_matrix,
emissivity_matrix (= the interface's coherent transmission), ft_even_diffuse_reflection_matrix."""
import numpy as np

from ..core.error import SMRTError
from ..core.substrate import SOIL_ARGUMENTS, SubstrateBase


class InterfaceSubstrate(SubstrateBase):
    interface_class = None          # set by the subclasses

    @property
    def device_kind(self):
        """The kind DORT evaluates on the device (smrt_batch.rough_kind): the interface model's.  For the grouping of the
        solvers the substrate stays a "host" object (core/snowpack.py: substrate_kind); DORT decides the route per group."""
        return getattr(self.interface, "device_kind", None)

    def device_params(self):
        return self.interface.device_params()

    def __init__(self, temperature=None, permittivity_model=None, **interface_parameters):
        soil = {k: interface_parameters.pop(k) for k in SOIL_ARGUMENTS if k in interface_parameters}
        super().__init__(temperature=temperature, permittivity_model=permittivity_model, **soil)
        self.interface = self.interface_class(**interface_parameters)
        for key in list(self.interface_class.args) + list(self.interface_class.optional_args):
            setattr(self, key, getattr(self.interface, key))

    def _below(self, frequency):
        eps = self.permittivity(frequency)
        if eps is None:
            raise SMRTError(f"No permittivity_model have been given to the substrate '{type(self).__name__}'")
        return eps

    def specular_reflection_matrix(self, frequency, eps_1, mu1, npol):
        return self.interface.specular_reflection_matrix(frequency, eps_1, self._below(frequency), mu1, npol)

    def emissivity_matrix(self, frequency, eps_1, mu1, npol):
        return self.interface.coherent_transmission_matrix(frequency, eps_1, self._below(frequency), mu1, npol)

    def diffuse_reflection_matrix(self, frequency, eps_1, mu_s, mu_i, dphi, npol):
        if not callable(getattr(self.interface, "diffuse_reflection_matrix", None)):
            return 0.0
        return self.interface.diffuse_reflection_matrix(frequency, eps_1, self._below(frequency), mu_s, mu_i, dphi, npol)

    def ft_even_diffuse_reflection_matrix(self, frequency, eps_1, mu_s, mu_i, m_max, npol):
        return self.interface.ft_even_diffuse_reflection_matrix(frequency, eps_1, self._below(frequency), mu_s, mu_i, m_max, npol)


class AdjustedFresnelSubstrate(SubstrateBase):
    """Substrates whose reflectivity is Fresnel's against the soil permittivity times a roughness factor per polarisation
    (soil_wegmuller, soil_qnh, rough_choudhury79): diagonal per stream, emissivity 1 - reflectivity, the third component
    left as Fresnel's.  The subclasses give `adjust(rv, rh, frequency, eps_1, mu1) -> (rv, rh)` on arrays and
    `device_tail() -> ((a0, a1), (c0, c1))`, the four numbers that follow the permittivities in substrate_p1 and
    substrate_p2 (include/smrt_dort.h).  The device evaluates them in passive mode; in active mode the objects go the host
    route through this protocol."""
    args = ()
    optional_args = {}

    def __init__(self, temperature=None, permittivity_model=None, **kwargs):
        for arg in self.args:
            if arg not in kwargs:
                raise SMRTError(f"Parameter {arg} must be specified")
            setattr(self, arg, kwargs.pop(arg))
        for arg, default in self.optional_args.items():
            setattr(self, arg, kwargs.pop(arg, default))
        super().__init__(temperature=temperature, permittivity_model=permittivity_model, **kwargs)

    def _below(self, frequency):
        eps = self.permittivity(frequency)
        if eps is None:
            raise SMRTError(f"No permittivity_model have been given to the substrate '{type(self).__name__}'")
        return eps

    def device_params(self, frequency):
        eps = complex(self._below(frequency))
        return eps.real, eps.imag

    def specular_reflection_matrix(self, frequency, eps_1, mu1, npol):
        from ..interface.fresnel import reflection_diagonal

        mu1 = np.atleast_1d(np.asarray(mu1, float))
        r = reflection_diagonal(eps_1, self._below(frequency), mu1, npol)
        r[0], r[1] = self.adjust(r[0], r[1], frequency, eps_1, mu1)
        return r

    def emissivity_matrix(self, frequency, eps_1, mu1, npol):
        from ..interface.fresnel import transmission_diagonal

        mu1 = np.atleast_1d(np.asarray(mu1, float))
        t = transmission_diagonal(eps_1, self._below(frequency), mu1, npol)
        rv, rh = self.adjust(1 - t[0], 1 - t[1], frequency, eps_1, mu1)
        t[0], t[1] = 1 - rv, 1 - rh
        return t


def ksigma(frequency, eps_1, roughness_rms):
    """Wavenumber in the last layer times the rms height, with the speed of light as soil_wegmuller.py:29 and
    rough_choudhury79.py:29 write it (2.9979e8, not C_SPEED: 4e-6 apart, which a brightness temperature at 1e-6 K sees)."""
    return (2 * np.pi * frequency * np.sqrt((1 / 2.9979e8) ** 2 * complex(eps_1)) * roughness_rms).real
