"""Multi-Fresnel Thermal Emission (MFTE) solver for passive sensors, MI355X-native (drop-in for
smrt/rtsolver/multifresnel_thermalemission.py).

The thermal emission of a stack of homogeneous, non-scattering layers with flat interfaces, characterised by their permittivity
and temperature alone (Hebert et al. 2015; annex of Zeiger et al. 2024): per sensor angle and polarisation the product of one
2 x 3 affine matrix per layer.  It is the solver for L-band over the dry zone of the ice sheets -- hundreds to thousands of
layers, many profiles, many angles -- where DORT diagonalises and eliminates for a problem that needs neither.

    m = make_model("nonscattering", "multifresnel_thermalemission")
    res = m.run(sensor_list.passive(1.4e9, [0, 40, 55]), snowpacks)
    res.TbV(), res.TbH()

The result has the dimensions (theta, polarization) with polarization V, H (the reference's order, not DORT's).  Any emmodel
with a device implementation works: only its effective permittivity is used, so "iba" gives the Tb of "nonscattering".
There is no Planck function: the temperatures are the physical ones.

prune_deep_snowpack (default 10; None: off) is the optical depth every angle starts with: the optical depth of a layer is
clipped, per angle, to what that angle has left (an angle that has run out still sees the interfaces), and the chain stops
after the first layer at which the steepest angle's remainder is negative.

Limits: passive sensors, Flat interfaces, no substrate / a Flat / a transparent one, no atmosphere, emmodels with a device
implementation, one GPU per call.

Deliberate differences from the reference: a Transparent substrate is no substrate with the shallow-snowpack warning
suppressed (the reference raises, although its own warning tells users to add one); prune_deep_snowpack=None really switches
the clipping off (the reference returns NaN); the two warnings are emitted once per run with a count.

The arithmetic runs in two HIP kernels through the C ABI (include/smrt_dort.h: smrt_multifresnel_*); packing of layers and
kinds is DORT's (rtsolver/dort.py).  A whole Model.run is one launch per homogeneous group (same angles, same substrate kind).
"""
import numpy as np

from ..core.error import SMRTError, smrt_warn
from ..core.snowpack import Snowpack, substrate_kind
from ..substrate.transparent import Transparent
from .dort import _Solution as _DortSolution, get_context
from .solver_base import RefusingPacker, SolverBase, check_error_handling


class MultiFresnelThermalEmission(SolverBase):
    """Options as smrt/rtsolver/multifresnel_thermalemission.py; `devices` (list of GPU indices; the first is used) is
    smrt_amd's own knob."""

    NAME = "MFTE"
    _broadcast_capability = {"theta", "polarization"}

    def __init__(self, error_handling="exception", prune_deep_snowpack=10, devices=None):
        check_error_handling(error_handling)
        if prune_deep_snowpack is not None:
            if isinstance(prune_deep_snowpack, (bool, str)) or not np.isscalar(prune_deep_snowpack):
                raise SMRTError("prune_deep_snowpack must be an optical depth or None")
            prune_deep_snowpack = float(prune_deep_snowpack)
            if not prune_deep_snowpack >= 0:
                raise SMRTError("prune_deep_snowpack must be non-negative (None switches pruning off)")
        self.error_handling = error_handling
        self.prune_deep_snowpack = prune_deep_snowpack
        self.devices = devices
        self.process_coherent_layers = False   # (read by DORT's result code)

    # ---- grouping, packing, launching ----------------------------------------------------------------------------
    @staticmethod
    def _check_sensor(sensor):
        if sensor.mode != "P":
            raise SMRTError("the MFTE solver is only suitable for passive microwave. Use an adequate sensor falling in this "
                            "category.")
        if np.ndim(sensor.frequency) != 0:
            raise SMRTError("the MFTE solver does not broadcast the frequency: split the sensor first (Model.run does)")

    @staticmethod
    def _sensor_key(sensor):
        return tuple(np.round(sensor.theta_deg, 12))

    def _packer(self):
        return _Packer(error_handling=self.error_handling, devices=self.devices, prune_deep_snowpack=None)

    @staticmethod
    def _check_snowpack(sp):
        """(the snowpack as it is packed, whether a missing substrate was asked for): a transparent substrate is no substrate."""
        if sp.atmosphere is not None:
            raise SMRTError("the MFTE solver can not handle atmosphere yet.")
        if not sp.all_interfaces_flat():
            raise SMRTError("Multi-Fresnel thermal emission only works with flat interfaces.")
        if isinstance(sp.substrate, Transparent):
            return Snowpack(layers=sp.layers, interfaces=sp.interfaces, substrate=None), True
        if sp.substrate is not None and substrate_kind(sp.substrate) != "flat":
            raise SMRTError("Multi-Fresnel thermal emission only works with flat substrates: "
                            f"{type(sp.substrate).__name__} is not implemented.")
        return sp, False

    def _snowpack_key(self, sp, on_host):
        if on_host:
            raise SMRTError("the MFTE solver has no route for emmodels evaluated on the host: use an emmodel with a device "
                            "implementation (nonscattering, iba, dmrt_qca_shortrange, dmrt_qcacp_shortrange)")
        sp, _ = self._check_snowpack(sp)
        return sp, substrate_kind(sp.substrate)

    def _context(self):
        return get_context((self.devices or [None])[0])   # (this module's name: the CPU tests put a stand-in here)

    def _solution(self, sensors, packs, sens_idx, pack_idx):
        return _Solution(self, sensors, packs, sens_idx, pack_idx)

    def _solve_indexed(self, sensors, packs, sens_idx, pack_idx, emmodel_names, packer=None):
        self._shallow, self._lossless = [], 0
        sol = SolverBase._solve_indexed(self, sensors, packs, sens_idx, pack_idx, emmodel_names, packer)
        self._warn(self._lossless, np.concatenate(self._shallow) if self._shallow else np.zeros(0))
        return sol

    def _launch(self, ctx, g):
        return ctx.multifresnel_run(g.batch, np.cos(g.sensor0.theta), self.prune_deep_snowpack, pairs=g.pairs)

    def _after_group(self, g, out):
        """What the two warnings of the run count."""
        if g.sps[0].substrate is not None:
            self._lossless += int(np.count_nonzero(g.batch.sub_p2.reshape(-1)[g.pair_of_row] < 1e-8))
        else:   # (a snowpack replaced before packing had a transparent substrate: the missing one was asked for)
            wanted_none = np.array([sp is not given for sp, given in zip(g.sps, g.given)])[g.pair_of_row % len(g.sps)]
            self._shallow.append(out.tau_snowpack[~wanted_none & np.all(out.status == 0, axis=1)])

    @staticmethod
    def _warn(lossless, tau):
        """The reference's two warnings, once per run with a count."""
        if lossless:
            smrt_warn(f"the permittivity of the substrate has a too small imaginary part for reliable results ({lossless} "
                      "simulation(s))")
        low = tau < 5
        if low.any():
            smrt_warn(f"Multifresnel has detected that the snowpack is optically shallow in {int(low.sum())} simulation(s) "
                      f"(smallest tau={np.nanmin(tau):g}) and no "
                      "substrate has been set, meaning that the space under the snowpack is 'empty' with snowpack shallow "
                      "enough to affect the measured signal at the surface. This is usually not wanted and can produce wrong "
                      "results. Either increase the thickness of the snowpack or set a substrate. If wanted, add a "
                      "transparent substrate to supress this warning")


class _Packer(RefusingPacker):
    SUBSTRATES_ON_HOST = "Multi-Fresnel thermal emission only works with flat substrates."
    INTERFACES_ON_HOST = "Multi-Fresnel thermal emission only works with flat interfaces."
    IBA_SCALARS_ON_HOST = EVALUATE_ON_HOST = "the MFTE solver has no route for emmodels evaluated on the host."


class _Solution(_DortSolution):
    """DORT's per-simulation and stacked results with this solver's dimensions."""

    def _coords(self, sensor):
        return [("theta", sensor.theta_deg), ("polarization", ["V", "H"])]
