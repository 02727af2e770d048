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

from .._native import STATUS_MESSAGES
from ..core.error import SMRTError
from ..core.snowpack import Snowpack, substrate_kind
from ..substrate.transparent import Transparent
from .dort import DORT, _Solution as _DortSolution, get_context


class SuccessiveOrder(object):
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
        if error_handling not in ("exception", "nan"):
            raise SMRTError("error_handling must be 'exception' or 'nan'")
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
        self.launches = 0      # launches of the last solve: tests assert "one launch per group"
        self.launch_info = []  # per launch: dict(chunks, reserved_bytes, over_budget, budget)

    # ---- the reference's protocol --------------------------------------------------------------------------------
    def solve(self, snowpack, emmodels, sensor, atmosphere=None, parallel_computation=None):
        from ..core.foreign import adopt_snowpack, entry_of_instance

        self._check_sensor(sensor)
        snowpack = adopt_snowpack(snowpack)
        if atmosphere is not None or snowpack.atmosphere is not None:
            raise SMRTError("the successive_order solver can not handle atmosphere yet.")
        if len(emmodels) != snowpack.nlayer:
            raise SMRTError("one emmodel per layer is needed")
        entries = [entry_of_instance(e, layer) for e, layer in zip(emmodels, snowpack.layers)]
        return self.solve_batch([(sensor, snowpack)], [entries])[0]

    def solve_batch(self, simulations, emmodel):
        """simulations: sequence of (single-frequency sensor, snowpack); one Result each (see DORT.solve_batch)."""
        from ..core.foreign import adopt_snowpack

        sensors, packs, si, pi = [], [], [], []
        seen_s, seen_p, memo = {}, {}, {}
        for sensor, sp in simulations:
            sp = adopt_snowpack(sp, memo)
            si.append(seen_s.setdefault(id(sensor), len(sensors)))
            if si[-1] == len(sensors):
                sensors.append(sensor)
            pi.append(seen_p.setdefault(id(sp), len(packs)))
            if pi[-1] == len(packs):
                packs.append(sp)
        if not si:
            return []
        names = emmodel if isinstance(emmodel, (list, str)) else DORT._device_name(emmodel)
        sol = self._solve_indexed(sensors, packs, np.asarray(si), np.asarray(pi), names)
        return [sol.result(i) for i in range(len(si))]

    def solve_plan(self, model, plan):
        """The whole plan of a Model.run, packed once and launched once per homogeneous group."""
        from ..core.model import nest_results

        for sensor in plan.sensors:
            self._check_sensor(sensor)
        packer = self._packer()
        packer._plan_facts = {id(sp): sp.layer_facts() for sp in plan.snowpacks}
        packer._plan_model = model
        try:
            names = DORT.emmodel_names(model, plan, packer._plan_facts)
            sol = self._solve_indexed(plan.sensors, plan.snowpacks, plan.sensor_index, plan.snowpack_index, names, packer)
        finally:
            packer._plan_facts = packer._plan_model = None
        stacked = sol.stacked_result(plan)
        if stacked is not None:
            return stacked
        return nest_results([sol.result(i) for i in range(len(plan))], plan.dimensions)

    emmodel_names = DORT.emmodel_names

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
    _NAME = "successive_order"

    @staticmethod
    def _sensor_key(sensor):
        """What must be uniform inside one launch, beyond the substrate kind."""
        return tuple(np.round(sensor.theta_deg, 12))

    def _context(self):
        return get_context((self.devices or [None])[0])

    @staticmethod
    def _solution_class():
        return _Solution

    def _run(self, ctx, batch, sensor0, pairs):
        """One launch (under the context lock): its output and its launch_info."""
        out = ctx.successive_order_run(batch, self.n_iteration_max, self.relative_tolerance, pairs=pairs,
                                       workspace_budget=self.workspace_budget)
        return out, ctx.successive_order_launch_info()

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
        if sp.substrate is not None and substrate_kind(sp.substrate) not in ("flat", "reflector"):
            raise SMRTError("the successive_order solver takes no substrate, a Flat, a Reflector or a transparent one: "
                            f"{type(sp.substrate).__name__} is not implemented.")
        return sp

    def _solve_indexed(self, sensors, packs, sens_idx, pack_idx, emmodel_names, packer=None):
        packer = packer or self._packer()
        sensor_keys, pack_keys = {}, {}
        s_code = np.empty(len(sensors), np.int64)
        for k, sensor in enumerate(sensors):
            self._check_sensor(sensor)
            s_code[k] = sensor_keys.setdefault(self._sensor_key(sensor), len(sensor_keys))
        p_code = np.empty(len(packs), np.int64)
        packed = []
        for k, sp in enumerate(packs):
            if not isinstance(emmodel_names, str) and any(not isinstance(e, str) for e in emmodel_names[k]):
                raise SMRTError(f"the {self._NAME} solver has no route for emmodels evaluated on the host: use an emmodel "
                                "with a device implementation (iba, dmrt_qca_shortrange, dmrt_qcacp_shortrange, nonscattering)")
            packed.append(self._check_snowpack(sp))
            if packed[-1] is not sp and packer._plan_facts is not None:
                packer._plan_facts[id(packed[-1])] = packer._plan_facts.get(id(sp))
            p_code[k] = pack_keys.setdefault(substrate_kind(packed[-1].substrate), len(pack_keys))
        freq = np.array([float(s.frequency) for s in sensors])
        code = s_code[sens_idx] * len(pack_keys) + p_code[pack_idx]
        sol = self._solution_class()(self, sensors, packs, sens_idx, pack_idx)
        ctx = self._context()
        self.launches, self.launch_info = 0, []
        for g in np.unique(code):
            sel = np.nonzero(code == g)[0]
            u_packs, inv_p = np.unique(pack_idx[sel], return_inverse=True)
            u_freq, inv_f = np.unique(freq[sens_idx[sel]], return_inverse=True)
            sensor0 = sensors[sens_idx[sel[0]]]
            sps = [packed[k] for k in u_packs]
            names = emmodel_names if isinstance(emmodel_names, str) else [emmodel_names[k] for k in u_packs]
            sensor_of = {float(sensors[k].frequency): sensors[k] for k in sens_idx[sel]}
            batch = packer._pack(sensor0, sps, u_freq, names, sensor_of)
            pairs = inv_f * len(u_packs) + inv_p
            full = len(pairs) == batch.n_pairs and np.array_equal(pairs, np.arange(batch.n_pairs))
            with ctx.lock:
                out, info = self._run(ctx, batch, sensor0, None if full else pairs)
                self.launch_info.append(info)
            self.launches += 1
            bad = np.nonzero(out.status != 0)[0]
            if len(bad) and self.error_handling == "exception":
                st = int(out.status[bad[0]])
                message = STATUS_MESSAGES.get(st, f"the {self._NAME} solver failed with status {st}")
                raise SMRTError(message.replace("N sublayers", f"{int(out.sublayers[bad[0]].sum())} sublayers"))
            sol.add_group(sel, out, sps[0], (u_packs, np.array(batch.n_layers, np.int64), np.array(batch.thickness, float)))
        return sol


class _Packer(DORT):
    """DORT's packing of layers and kinds for this solver; everything DORT would evaluate on the host is refused."""

    def _substrates_on_host(self, *args, **kwargs):
        raise SMRTError("the successive_order solver takes no substrate, a Flat, a Reflector or a transparent one.")

    def _interfaces_on_host(self, *args, **kwargs):
        raise SMRTError("the successive_order solver takes Flat interfaces only: rough interfaces are not implemented.")

    def _iba_scalars_on_host(self, *args, **kwargs):
        raise SMRTError("the successive_order solver has no route for emmodels evaluated on the host.")

    def _evaluate_on_host(self, *args, **kwargs):
        raise SMRTError("the successive_order solver has no route for emmodels evaluated on the host.")


class _Solution(_DortSolution):
    """DORT's per-simulation and stacked results with the trailing `order` dimension."""

    def _coords(self, sensor):
        order = np.empty(self.solver.n_iteration_max + 1, dtype=object)
        order[:-1] = list(range(self.solver.n_iteration_max))
        order[-1] = "total"
        return [("polarization", ["V", "H"]), ("theta", sensor.theta_deg), ("order", order)]
