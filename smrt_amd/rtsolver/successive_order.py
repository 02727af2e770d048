"""Successive-order-of-scattering solver for passive sensors, MI355X-native (drop-in for smrt/rtsolver/successive_order.py).

A multi-stream solver on the same discrete ordinates as DORT (Lenoble et al. 2007, eq. 66; Greenwald et al. 2005, eq. 2):
every layer is cut into sublayers of optical depth <= 0.1, the radiance at every sub-interface is swept down and up once per
order, and the scattering of one order is the source of the next.  No eigenproblem, so it answers where DORT's
diagonalisation fails, and it returns the brightness temperature ORDER BY ORDER: emission alone (order 0), single
scattering (order 1), ...  Truncated at a low order it is the cheap solver of Greenwald et al.

    m = make_model("iba", "successive_order", rtsolver_options={"n_max_stream": 8, "n_iteration_max": 12})
    res = m.run(sensor_list.passive(37e9, 55), sp)
    res.TbV(order="total"), res.TbV(order=0)

The result has the dimensions (polarization, theta, order); `order` is 0 .. n_iteration_max - 1 followed by "total".  Every
order goes through the inverse Planck function by itself, the total is the inverse Planck function of the summed radiances
(as in the reference).  The loop stops after storing the first order whose largest emerging radiance is below
relative_tolerance x that of order 0; later orders are exactly 0.

Limits: passive sensors, Flat interfaces, no substrate / Flat / Reflector / transparent substrate, no atmosphere, emmodels
with a device implementation, no process_coherent_layers, no phase_symmetrization, 2 to 64 streams.

Three deliberate differences from the reference: the emission (1 - R) B(T) of the substrate enters order 0 (the reference
leaves it out in passive mode); an atmosphere raises SMRTError (the reference crashes); only mode 0 of the phase matrix is
computed, so the Rayleigh-family emmodels work with the default m_max (the reference crashes) -- m_max only sets the number
of azimuth samples of IBA's phase function, as it does in the reference.

The arithmetic runs in three HIP kernels through the C ABI (include/smrt_dort.h: smrt_successive_order_*); packing of
layers and kinds is DORT's (rtsolver/dort.py).  A whole Model.run is one launch per homogeneous group.
"""
import numpy as np

from ..core.error import SMRTError
from ..core.snowpack import Snowpack, substrate_kind
from ..core.substrate import PASSIVE_DEVICE_KINDS
from ..substrate.transparent import Transparent
from .dort import _Solution as _DortSolution, get_context
from .solver_base import RefusingPacker, SolverBase, check_error_handling


class SuccessiveOrder(SolverBase):
    """Options as smrt/rtsolver/successive_order.py; `devices` (list of GPU indices; the first is used) and
    `workspace_budget` (bytes the solver may reserve on the device; None: the library's default of 8 GiB) are smrt_amd's own
    knobs."""

    _broadcast_capability = {"theta_inc", "polarization_inc", "theta", "phi", "polarization"}

    def __init__(self, n_max_stream=32, n_iteration_max=50, relative_tolerance=0.001, m_max=2, stream_mode="most_refringent",
                 phase_symmetrization=False, error_handling="exception", process_coherent_layers=False,
                 incident_polarizations="VH", rayleigh_jeans_approximation=False, devices=None, workspace_budget=None):
        if stream_mode != "most_refringent":
            raise SMRTError("smrt_amd's successive_order solver implements stream_mode='most_refringent' only")
        if phase_symmetrization:
            raise SMRTError("phase_symmetrization is not available in the successive_order solver (the reference itself warns "
                            "that it may not work)")
        if process_coherent_layers:
            raise SMRTError("process_coherent_layers is not available in the successive_order solver")
        check_error_handling(error_handling)
        if incident_polarizations not in ("V", "VH", "VHU"):
            raise SMRTError("The argument incident_polarizations must be V, VH or VHU. Note that H only is not supported yet.")
        if not 2 <= int(n_max_stream) <= 64:
            raise SMRTError("the successive_order solver takes 2 to 64 streams (n_max_stream)")
        if int(n_iteration_max) < 1:
            raise SMRTError("n_iteration_max must be at least 1")
        if not float(relative_tolerance) >= 0:
            raise SMRTError("relative_tolerance must be non-negative")
        if int(m_max) < 0:
            raise SMRTError("m_max must be non-negative")
        self.n_max_stream = int(n_max_stream)
        self.n_iteration_max = int(n_iteration_max)
        self.relative_tolerance = float(relative_tolerance)
        self.m_max = int(m_max)
        self.stream_mode = stream_mode
        self.phase_symmetrization = False
        self.error_handling = error_handling
        self.process_coherent_layers = False
        self.incident_polarizations = incident_polarizations
        self.rayleigh_jeans_approximation = bool(rayleigh_jeans_approximation)
        self.devices = devices
        self.workspace_budget = workspace_budget
        self.launch_info = []

    # ---- grouping, packing, launching ----------------------------------------------------------------------------
    @staticmethod
    def _check_sensor(sensor):
        if sensor.mode != "P":
            raise SMRTError("the successive_order solver of smrt_amd is only suitable for passive microwave: active sensors "
                            "are not implemented here, use rtsolver 'successive_order_backscatter'.")
        if np.ndim(sensor.frequency) != 0:
            raise SMRTError("the successive_order solver does not broadcast the frequency: split the sensor first "
                            "(Model.run does)")

    # what the active sibling (rtsolver/successive_order_backscatter.py) replaces; the grouping and the pair map are shared
    NAME = "successive_order"
    ATMOSPHERE = "the successive_order solver can not handle atmosphere yet."   # (solve: the active sibling says it in these words too)

    @staticmethod
    def _sensor_key(sensor):
        """What must be uniform inside one launch, beyond the substrate kind."""
        return tuple(np.round(sensor.theta_deg, 12))

    def _context(self):
        return get_context((self.devices or [None])[0])   # (this module's name: the CPU tests put a stand-in here)

    def _solution(self, sensors, packs, sens_idx, pack_idx):
        return _Solution(self, sensors, packs, sens_idx, pack_idx)

    def _launch(self, ctx, g):
        out = ctx.successive_order_run(g.batch, self.n_iteration_max, self.relative_tolerance, pairs=g.pairs,
                                       workspace_budget=self.workspace_budget)
        self.launch_info.append(ctx.successive_order_launch_info())
        return out

    def _packer(self):
        return _Packer(n_max_stream=self.n_max_stream, m_max=self.m_max, error_handling=self.error_handling,
                       rayleigh_jeans_approximation=self.rayleigh_jeans_approximation, devices=self.devices)

    @staticmethod
    def _check_snowpack(sp):
        """The snowpack as it is packed: a transparent substrate is no substrate."""
        if sp.atmosphere is not None:
            raise SMRTError("the successive_order solver can not handle atmosphere yet.")
        if not sp.all_interfaces_flat():
            raise SMRTError("the successive_order solver takes Flat interfaces only: rough interfaces are not implemented.")
        if isinstance(sp.substrate, Transparent):
            return Snowpack(layers=sp.layers, interfaces=sp.interfaces, substrate=None)
        if sp.substrate is not None and substrate_kind(sp.substrate) not in ("flat", "reflector") + PASSIVE_DEVICE_KINDS:
            raise SMRTError("the successive_order solver takes no substrate, a Flat, a Reflector or a transparent one: "
                            f"{type(sp.substrate).__name__} is not implemented.")
        return sp

    def _snowpack_key(self, sp, on_host):
        if on_host:
            raise SMRTError(f"the {self.NAME} solver has no route for emmodels evaluated on the host: use an emmodel "
                            "with a device implementation (iba, dmrt_qca_shortrange, dmrt_qcacp_shortrange, nonscattering)")
        sp = self._check_snowpack(sp)
        return sp, substrate_kind(sp.substrate)

    def _status_message(self, out, at, status):
        return SolverBase._status_message(self, out, at, status).replace("N sublayers", f"{int(out.sublayers[at].sum())} sublayers")


class _Packer(RefusingPacker):
    SUBSTRATES_ON_HOST = "the successive_order solver takes no substrate, a Flat, a Reflector or a transparent one."
    INTERFACES_ON_HOST = "the successive_order solver takes Flat interfaces only: rough interfaces are not implemented."
    IBA_SCALARS_ON_HOST = EVALUATE_ON_HOST = "the successive_order solver has no route for emmodels evaluated on the host."


class _Solution(_DortSolution):
    """DORT's per-simulation and stacked results with the trailing `order` dimension."""

    def _coords(self, sensor):
        order = np.empty(self.solver.n_iteration_max + 1, dtype=object)
        order[:-1] = list(range(self.solver.n_iteration_max))
        order[-1] = "total"
        return [("polarization", ["V", "H"]), ("theta", sensor.theta_deg), ("order", order)]
