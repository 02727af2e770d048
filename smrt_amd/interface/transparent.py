"""Transparent interface (smrt/interface/transparent.py): reflects nothing and transmits everything, whatever the two
media.  Evaluated on the host through the interface protocol; the iterative first-order solver and analytic checks of a
volume-scattering term alone use it."""
import numpy as np


class Transparent:
    args = []
    optional_args = {}

    def specular_reflection_matrix(self, frequency, eps_1, eps_2, mu1, npol):
        return np.zeros((npol, len(np.atleast_1d(mu1))))

    def diffuse_reflection_matrix(self, frequency, eps_1, eps_2, mu_s, mu_i, dphi, npol):
        return 0.0

    def ft_even_diffuse_reflection_matrix(self, frequency, eps_1, eps_2, mu_s, mu_i, m_max, npol):
        return 0.0

    def coherent_transmission_matrix(self, frequency, eps_1, eps_2, mu1, npol):
        return np.ones((npol, len(np.atleast_1d(mu1))))

    def diffuse_transmission_matrix(self, frequency, eps_1, eps_2, mu_s, mu_i, dphi, npol):
        return 0.0

    def ft_even_diffuse_transmission_matrix(self, frequency, eps_1, eps_2, mu_s, mu_i, m_max, npol):
        return 0.0
