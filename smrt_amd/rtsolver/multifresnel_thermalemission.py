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

from .._native import STATUS_MESSAGES
from ..core.error import SMRTError, smrt_warn
from ..core.snowpack import Snowpack, substrate_kind
from ..substrate.transparent import Transparent
from .dort import DORT, _Solution as _DortSolution, get_context


class MultiFresnelThermalEmission(object):
    """Options as smrt/rtsolver/multifresnel_thermalemission.py; `devices` (list of GPU indices; the first is used) is
    smrt_amd's own knob."""

    _broadcast_capability = {"theta", "polarization"}

    def __init__(self, error_handling="exception", prune_deep_snowpack=10, devices=None):
        if error_handling not in ("exception", "nan"):
            raise SMRTError("error_handling must be 'exception' or 'nan'")
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
        self.launches = 0                      # launches of the last solve: tests assert "one launch per group"

    # ---- the reference's protocol --------------------------------------------------------------------------------
    def solve(self, snowpack, emmodels, sensor, atmosphere=None, parallel_computation=None):
        from ..core.foreign import adopt_snowpack, entry_of_instance

        self._check_sensor(sensor)
        snowpack = adopt_snowpack(snowpack)
        if atmosphere is not None or snowpack.atmosphere is not None:
            raise SMRTError("the MFTE solver can not handle atmosphere yet.")
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
            raise SMRTError("the MFTE solver is only suitable for passive microwave. Use an adequate sensor falling in this "
                            "category.")
        if np.ndim(sensor.frequency) != 0:
            raise SMRTError("the MFTE solver does not broadcast the frequency: split the sensor first (Model.run does)")

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

    def _solve_indexed(self, sensors, packs, sens_idx, pack_idx, emmodel_names, packer=None):
        packer = packer or self._packer()
        sensor_keys, pack_keys = {}, {}
        s_code = np.empty(len(sensors), np.int64)
        for k, sensor in enumerate(sensors):
            self._check_sensor(sensor)
            s_code[k] = sensor_keys.setdefault(tuple(np.round(sensor.theta_deg, 12)), len(sensor_keys))
        p_code = np.empty(len(packs), np.int64)
        packed, wanted_none = [], np.zeros(len(packs), bool)
        for k, sp in enumerate(packs):
            if not isinstance(emmodel_names, str) and any(not isinstance(e, str) for e in emmodel_names[k]):
                raise SMRTError("the MFTE solver has no route for emmodels evaluated on the host: use an emmodel with a device "
                                "implementation (nonscattering, iba, dmrt_qca_shortrange, dmrt_qcacp_shortrange)")
            checked, wanted_none[k] = self._check_snowpack(sp)
            packed.append(checked)
            if checked is not sp and packer._plan_facts is not None:
                packer._plan_facts[id(checked)] = packer._plan_facts.get(id(sp))
            p_code[k] = pack_keys.setdefault(substrate_kind(checked.substrate), len(pack_keys))
        freq = np.array([float(s.frequency) for s in sensors])
        code = s_code[sens_idx] * len(pack_keys) + p_code[pack_idx]
        sol = _Solution(self, sensors, packs, sens_idx, pack_idx)
        ctx = get_context((self.devices or [None])[0])
        self.launches = 0
        shallow, lossless = [], 0
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
                out = ctx.multifresnel_run(batch, np.cos(sensor0.theta), self.prune_deep_snowpack, pairs=None if full else pairs)
            self.launches += 1
            if sps[0].substrate is not None:
                lossless += int(np.count_nonzero(batch.sub_p2.reshape(-1)[pairs] < 1e-8))
            else:
                shallow.append(out.tau_snowpack[~wanted_none[pack_idx[sel]] & np.all(out.status == 0, axis=1)])
            bad = np.argwhere(out.status != 0)
            if len(bad) and self.error_handling == "exception":
                st = int(out.status[tuple(bad[0])])
                raise SMRTError(STATUS_MESSAGES.get(st, f"the MFTE solver failed with status {st}"))
            sol.add_group(sel, out, sps[0], (u_packs, np.array(batch.n_layers, np.int64), np.array(batch.thickness, float)))
        self._warn(lossless, np.concatenate(shallow) if shallow else np.zeros(0))
        return sol

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


class _Packer(DORT):
    """DORT's packing of layers and kinds for this solver; everything DORT would evaluate on the host is refused."""

    def _substrates_on_host(self, *args, **kwargs):
        raise SMRTError("Multi-Fresnel thermal emission only works with flat substrates.")

    def _interfaces_on_host(self, *args, **kwargs):
        raise SMRTError("Multi-Fresnel thermal emission only works with flat interfaces.")

    def _iba_scalars_on_host(self, *args, **kwargs):
        raise SMRTError("the MFTE solver has no route for emmodels evaluated on the host.")

    def _evaluate_on_host(self, *args, **kwargs):
        raise SMRTError("the MFTE solver has no route for emmodels evaluated on the host.")


class _Solution(_DortSolution):
    """DORT's per-simulation and stacked results with this solver's dimensions."""

    def _coords(self, sensor):
        return [("theta", sensor.theta_deg), ("polarization", ["V", "H"])]
