"""Successive-order-of-scattering solver for ACTIVE sensors, MI355X-native: the active mode of smrt/rtsolver/successive_order.py.

Backscatter ORDER BY ORDER on the same discrete ordinates as DORT, without an eigenproblem: order 0 is the coherent part
(removed, as in DORT), order 1 single scattering (volume or interface), order 2 double scattering, ...  It sits between
`iterative_first_order` (closed form, stops at order 1) and `dort` (everything, no split by order).

    m = make_model("iba", "successive_order_backscatter", rtsolver_options={"n_max_stream": 16, "n_iteration_max": 8})
    res = m.run(sensor_list.active(13e9, [30, 50]), sp)
    res.sigmaVV(order="total"), res.sigmaVV_dB(order=1), res.sigmaHV_dB(order=2)

The result has the dimensions of the active DORT result (polarization_inc, polarization, theta_inc) and a trailing `order`:
0 .. n_iteration_max - 1 followed by "total".  Inside smrt-model/smrt ONE class, SuccessiveOrder, serves both sensor modes;
here it is two names, `successive_order` (passive) and `successive_order_backscatter` (active): the two modes share no
kernel, and the passive solver's refusal of active sensors is part of its tested behaviour.

The arithmetic follows the reference as written: three polarisations everywhere; one coherent pass (no phase matrix, every
order) and one pass per azimuth mode 0 .. m_max; a mode pass stops after storing the first order whose largest emerging
radiance is below relative_tolerance x that of mode 0 at order 0; (1 + [m > 0]) x the coherent orders are subtracted from
ALL orders of a mode, so the orders after a stop hold minus the coherent remainder (below the tolerance) and not 0.

Limits: active sensors at backscatter (theta == theta_inc, scalar phi), Flat interfaces, no substrate / Flat / transparent
substrate (a Reflector has no third Stokes component, in the reference neither), no atmosphere, emmodels with a device
implementation, no process_coherent_layers, no phase_symmetrization, stream_mode "most_refringent", 2 to 64 streams, m_max at
most 2 with the Rayleigh-family emmodels.

The arithmetic runs in four HIP kernels through the C ABI (include/smrt_dort.h: smrt_so_active_*); packing of layers and
kinds is DORT's (rtsolver/dort.py).  A whole Model.run is one launch per homogeneous group (same incidence angles, same
substrate kind).
"""
import numpy as np

from ..core.error import SMRTError
from ..core.snowpack import Snowpack, substrate_kind
from ..substrate.transparent import Transparent
from .dort import get_context
from .successive_order import SuccessiveOrder as _PassiveSuccessiveOrder, _Solution as _PassiveSolution


class SuccessiveOrderBackscatter(_PassiveSuccessiveOrder):
    """Options as smrt/rtsolver/successive_order.py (rayleigh_jeans_approximation has no effect in active mode); `devices`
    and `workspace_budget` as in the passive solver.  solve, solve_batch and solve_plan are the passive solver's."""

    # ---- grouping, packing, launching ----------------------------------------------------------------------------
    @staticmethod
    def _check_sensor(sensor):
        if sensor.mode != "A":
            raise SMRTError("the successive_order_backscatter solver is only suitable for active microwave: use rtsolver "
                            "'successive_order' for passive sensors.")
        if np.ndim(sensor.frequency) != 0:
            raise SMRTError("the successive_order_backscatter solver does not broadcast the frequency: split the sensor first "
                            "(Model.run does)")
        if np.size(sensor.phi) > 1:
            raise SMRTError("phi as an array must be implemented")
        if not np.array_equal(sensor.theta_deg, sensor.theta_inc_deg):
            raise SMRTError("the successive_order_backscatter solver computes the backscatter (theta == theta_inc)")

    @staticmethod
    def _check_snowpack(sp):
        """The snowpack as it is packed: a transparent substrate is no substrate."""
        if sp.atmosphere is not None:
            raise SMRTError("the successive_order_backscatter solver can not handle atmosphere yet.")
        if not sp.all_interfaces_flat():
            raise SMRTError("the successive_order_backscatter solver takes Flat interfaces only: rough interfaces are not implemented.")
        if isinstance(sp.substrate, Transparent):
            return Snowpack(layers=sp.layers, interfaces=sp.interfaces, substrate=None)
        if sp.substrate is not None and substrate_kind(sp.substrate) != "flat":
            raise SMRTError("the successive_order_backscatter solver takes no substrate, a Flat or a transparent one: "
                            f"{type(sp.substrate).__name__} is not implemented.")
        return sp

    # ---- the other hooks the passive solver's differ in (grouping, packing and the pair map are shared) ------------------
    NAME = "successive_order_backscatter"

    @staticmethod
    def _sensor_key(sensor):
        return (tuple(np.round(sensor.theta_inc_deg, 12)), float(np.ravel(sensor.phi)[0]))

    def _context(self):
        return get_context((self.devices or [None])[0])   # (this module's name: the CPU tests put a stand-in here)

    def _solution(self, sensors, packs, sens_idx, pack_idx):
        return _Solution(self, sensors, packs, sens_idx, pack_idx)

    def _launch(self, ctx, g):
        out = ctx.so_active_run(g.batch, np.atleast_1d(g.sensor0.theta_inc), self.n_iteration_max, self.relative_tolerance,
                                incident_npol=len(self.incident_polarizations), m_max=self.m_max, pairs=g.pairs,
                                workspace_budget=self.workspace_budget)
        self.launch_info.append(ctx.so_active_launch_info())
        return out


class _Solution(_PassiveSolution):
    """DORT's per-simulation and stacked active results with the trailing `order` dimension."""

    def _coords(self, sensor):
        pola = ["V", "H", "U"]
        return [("polarization_inc", pola), ("polarization", pola), ("theta_inc", sensor.theta_inc_deg),
                _PassiveSolution._coords(self, sensor)[-1]]
