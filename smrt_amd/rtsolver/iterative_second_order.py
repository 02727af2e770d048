"""Iterative second-order backscatter solver, MI355X-native (drop-in for smrt/rtsolver/iterative_second_order.py, after
Karam et al. 1995).

For radar users of `iterative_first_order` who need a cross-polarised volume return -- first order gives exactly zero HV /
VH in its volume terms -- or who want to judge whether first order is enough for their snow.  Besides the contributions of
the first order it splits off three more mechanisms:

* ``order2_intralayer_scattering``: two volume scatterings inside one layer;
* ``order2_rough_layer_scattering``: one volume scattering combined with the diffuse reflection of a rough substrate (needs
  a substrate with the full bistatic ``ft_even_diffuse_reflection_matrix``: ``geometrical_optics``);
* ``order2_interlayer_scattering``: two volume scatterings in two different layers (``compute_scattering_interlayer=True``;
  O(L^2) work).

    m = make_model("iba", "iterative_second_order", rtsolver_options={"return_contributions": True})
    res = m.run(sensor_list.active(13e9, [20, 35, 50]), snowpacks)
    res.sigmaHV_dB(), res.sigmaVV_dB(contribution="order2_intralayer_scattering")

Options as the reference's: error_handling, return_contributions, n_max_stream=32 (quadrature cosines per layer),
stream_mode="most_refringent" (the only one), m_max=5 (azimuth modes 0 .. m_max - 1 are summed; at most 8),
compute_scattering_interlayer=False; `devices` is smrt_amd's own knob.

Orders 0 and 1 are the first-order solver's kernels, bit for bit.  The order-2 integrals run in HIP kernels of their own
(include/smrt_dort.h: smrt_second_order_*; smrt_amd/csrc/second_order_kernel.hpp): stream sets per (pair, layer), one
wavefront per (pair, layer, angle) -- per (pair, layer, layer, angle) for the interlayer term -- with the streams on the
lanes, and a walk per (pair, angle).  As in first order, interface and substrate objects the device does not know are
evaluated here and handed over as numbers; the substrate's diffuse reflection modes are evaluated at the cosines the device
will use (the layer's stream set is restated here).

Limits: everything of `iterative_first_order` (backscatter, active, V and H, no atmosphere, albedo below about 0.5), and
* an inner interface with diffuse reflection is refused: the solver has no term for it (the reference's term needs a full
  bistatic matrix that its own rough interfaces do not provide);
* emmodels evaluated on the host (outside the IBA and Rayleigh families and non-scattering layers) are refused, before
  any of them is evaluated;
* a Transparent inner interface is accepted but, like every interface object other than Flat, evaluated here and handed
  over as numbers (first order's interface slots), not on the device.

Deliberate differences from the reference: the warnings are emitted once per run (first order's rule); where a quadrature
cosine equals the incidence cosine in the layer exactly, the reference's 0 / 0 is replaced by the analytic limit.  Findings
reproduced as they are: mode m_max is computed but never summed; the interlayer term pairs streams by
index, uses layer n's cosines in every attenuation factor and counts both end layers in the intermediate optical depth -- it
can be negative.
"""
import numpy as np

from .._native import PackedSecondOrderExtras
from ..core.error import SMRTError
from ..core.snowpack import substrate_kind
from ..interface.flat import Flat
from ..interface.transparent import Transparent
from .iterative_first_order import CONTRIBUTIONS as FIRST_ORDER_CONTRIBUTIONS
from .iterative_first_order import IterativeFirstOrder, _Packer, _Solution

CONTRIBUTIONS = FIRST_ORDER_CONTRIBUTIONS + ["order2_intralayer_scattering", "order2_rough_layer_scattering",
                                             "order2_interlayer_scattering"]
NAME = "iterative_second_order"
STREAM_MARGIN = 1e-9   # see IterativeSecondOrder.stream_sets


class IterativeSecondOrder(IterativeFirstOrder):
    """See the module.  `devices`: list of GPU indices (the first is used); `workspace_budget`: bytes the order-2 buffers stay
    inside on the device (None: the library's default; the launch works chunk after chunk)."""

    NAME = NAME

    def __init__(self, error_handling="exception", return_contributions=False, n_max_stream=32, stream_mode="most_refringent",
                 m_max=5, compute_scattering_interlayer=False, devices=None, workspace_budget=None):
        IterativeFirstOrder.__init__(self, error_handling, return_contributions, devices)
        if stream_mode not in (None, "most_refringent"):
            raise SMRTError(f"stream_mode '{stream_mode}' is not supported on the device: only 'most_refringent' is implemented")
        if int(n_max_stream) < 2:
            raise SMRTError("n_max_stream must be at least 2")
        if not 1 <= int(m_max) <= 8:
            raise SMRTError("m_max must be 1 to 8")
        self.n_max_stream, self.m_max, self.stream_mode = int(n_max_stream), int(m_max), "most_refringent"
        self.compute_scattering_interlayer = bool(compute_scattering_interlayer)
        self.workspace_budget = workspace_budget

    def _packer(self):
        return _SecondOrderPacker(n_max_stream=self.n_max_stream, m_max=self.m_max, error_handling=self.error_handling,
                                  devices=self.devices)

    def _solve_indexed(self, sensors, packs, sens_idx, pack_idx, emmodel_names, packer=None):
        for sp in packs:
            for i, itf in enumerate(sp.interfaces[1:], 1):
                if not isinstance(itf, (Flat, Transparent)):
                    raise SMRTError(f"the {NAME} solver has no term for diffuse reflection at an inner interface: interface {i} "
                                    f"({type(itf).__name__}) must be Flat or Transparent. Only the surface and the substrate may be rough.")
        return IterativeFirstOrder._solve_indexed(self, sensors, packs, sens_idx, pack_idx, emmodel_names, packer)

    def _run_group(self, ctx, batch, extras, pairs, packer, sensor0, sps, freqs):
        modes = self._substrate_modes(ctx, batch, sensor0, sps, freqs)
        x = PackedSecondOrderExtras(batch, self.compute_scattering_interlayer, self.workspace_budget, extras, modes)
        return ctx.second_order_run(batch, x, pairs=pairs)

    # ---- what the host evaluates beyond first order ----------------------------------------------------------------
    @staticmethod
    def stream_sets(n_max_stream, eps):
        """[(cosines ascending, weights)] per layer: Gauss-Legendre nodes of the most refringent layer carried over by
        Snell's law, total reflections dropped, finite-difference weights -- as the device computes them.

        The host and the device must keep the same NUMBER of streams in every layer, or the substrate rows evaluated here
        would sit one stream off.  Both test `relsin < 1` on numbers that agree to rounding only (scipy's nodes and NumPy's
        square roots here; the library's own Gauss-Legendre table and the device's sqrt there), so a node whose relative
        sine lies within STREAM_MARGIN of 1 is refused here: the two sides cannot differ outside that margin, which is a
        million times their rounding and still a set of inputs nobody meets."""
        from scipy.special import roots_legendre

        eps = np.asarray(eps, complex)
        star = eps[int(np.argmax(eps))]
        node = roots_legendre(2 * n_max_stream)[0][-1:n_max_stream - 1:-1]
        sets = []
        for e in eps:
            relsin = np.sqrt(star / e).real * np.sqrt(1.0 - node ** 2)
            if (np.abs(relsin - 1.0) < STREAM_MARGIN).any():
                raise SMRTError(f"the {NAME} solver cannot tell whether a stream of a layer (permittivity {e:g} under {star:g}) is "
                                "totally reflected: its relative sine is 1 to rounding, and the substrate's diffuse reflection "
                                "evaluated on the host could be misaligned with the device's streams. Change n_max_stream.")
            mu = np.sqrt(1.0 - relsin[relsin < 1.0] ** 2)
            w = np.empty_like(mu)
            if len(mu) >= 2:
                w[0], w[-1] = 1.0 - 0.5 * (mu[0] + mu[1]), 0.5 * (mu[-2] + mu[-1])
                w[1:-1] = 0.5 * (mu[:-2] - mu[2:])
            sets.append((mu[::-1], np.abs(w)[::-1]))
        return sets

    @staticmethod
    def substrate_rows(substrate, frequency, eps_last, mu_i, mu_int, m_max):
        """[len(mu_int), m_max, 2, 2, 3] of a substrate object for one incidence cosine: rows V, H of its diffuse reflection
        modes at (scattered -mu_i, incident mu') and (scattered mu', incident mu_i), called as the reference calls it."""
        a, b = np.array([-mu_i, mu_i]), np.concatenate([-mu_int, mu_int])
        n = len(mu_int)
        out = np.zeros((n, m_max, 2, 2, 3))
        r1 = substrate.ft_even_diffuse_reflection_matrix(frequency, eps_last, a, b, m_max, 3)
        r2 = substrate.ft_even_diffuse_reflection_matrix(frequency, eps_last, b, a, m_max, 3)
        r1, r2 = (np.asarray(getattr(r, "values", r), float) for r in (r1, r2))
        if r1.ndim == 0 and r2.ndim == 0 and r1 == 0.0 and r2 == 0.0:
            return out
        if r1.shape != (3, 3, m_max + 1, 2, 2 * n) or r2.shape != (3, 3, m_max + 1, 2 * n, 2):
            raise SMRTError(f"the {NAME} solver needs dense diffuse reflection modes [3, 3, m_max + 1, mu_s, mu_i] of the "
                            f"substrate, got {r1.shape} and {r2.shape}")
        out[:, :, 0] = np.transpose(r1[:2, :, :m_max, 0, n:], (3, 2, 0, 1))
        out[:, :, 1] = np.transpose(r2[:2, :, :m_max, n:, 1], (3, 2, 0, 1))
        return out

    def _substrate_modes(self, ctx, batch, sensor0, sps, freqs):
        subs = [sp.substrate for sp in sps]
        rough = [s is not None and substrate_kind(s, "A") == "host" and callable(getattr(s, "ft_even_diffuse_reflection_matrix", None))
                 for s in subs]
        if not any(rough):
            return None
        F, S, Lmax = len(freqs), len(sps), int(batch.struct.n_layers_max)
        mu0 = np.cos(np.atleast_1d(sensor0.theta_inc))
        lay = np.asarray(ctx.first_order_layers(batch)).reshape(F, S, Lmax, 5)
        self.launches += 1
        modes = np.zeros((F, S, Lmax, len(mu0), self.n_max_stream, self.m_max, 2, 2, 3))
        for fi, f in enumerate(freqs):
            for s, sp in enumerate(sps):
                if not rough[s]:
                    continue
                L = sp.nlayer
                eps = lay[fi, s, :L, 0] + 1j * lay[fi, s, :L, 1]
                for l, (mu_int, _) in enumerate(self.stream_sets(self.n_max_stream, eps)):
                    if lay[fi, s, l, 2] == 0.0 or len(mu_int) < 2:
                        continue
                    for t, mi in enumerate(self.snell_from_air(eps[l], mu0)):
                        modes[fi, s, l, t, :len(mu_int)] = self.substrate_rows(sp.substrate, float(f), eps[L - 1], mi, mu_int, self.m_max)
        return modes

    def _solution(self, sensors, packs, sens_idx, pack_idx):
        return _SecondOrderSolution(self, sensors, packs, sens_idx, pack_idx)


class _SecondOrderPacker(_Packer):
    """First order's packing, without the route for emmodels evaluated on the host: refused before any of them is
    evaluated.  (Emmodels of the IBA and Rayleigh families that hand over their scalars only keep their route: their phase
    modes are the device's.)"""

    def _evaluate_on_host(self, *args, **kwargs):
        raise SMRTError(f"the {NAME} solver cannot use emmodels evaluated on the host: only the IBA family, the Rayleigh "
                        "family and non-scattering layers have their phase modes on the device")


class _SecondOrderSolution(_Solution):
    def _coords(self, sensor):
        coords = _Solution._coords(self, sensor)
        return ([("contribution", CONTRIBUTIONS)] + coords[1:]) if self.solver.return_contributions else coords

    def _values(self, values):
        """[..., 7, n, 2, 2] -> the total, or [..., 8, n, 2, 2] with the total first."""
        total = values[..., 0, :, :, :]
        for c in range(1, 7):
            total = total + values[..., c, :, :, :]
        if not self.solver.return_contributions:
            return total
        return np.concatenate([total[..., None, :, :, :], values], axis=-4)
