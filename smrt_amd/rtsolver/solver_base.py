"""What the solvers beside DORT share on the Python side (the C++ side of the same idea: csrc/solver_host.hpp).

* `SolverBase`: the reference's protocol (solve, solve_batch, solve_plan, emmodel_names) and the loop over the homogeneous groups
  of a run -- codes per sensor and per snowpack, one packed batch and one launch per group, the map from simulations to the
  pairs of the batch, the status words turned into an SMRTError -- written once, with the hooks listed in the class.
* `RefusingPacker`: DORT's packing for a solver that has nothing evaluated on the host.
* `LayeredSolution`: dort._Solution for the solvers whose diagnostics are the layer scalars alone (no streams).
* the checks of the options every solver takes, and the two pieces of host arithmetic the altimetry solvers share.

A new solver writes: its options, `_check_sensor`, `_sensor_key`, `_packer`, `_launch` and the coordinates of its result; the
other hooks when it replaces snowpacks, evaluates something on the host or collects warnings.
"""
import types

import numpy as np

from . import dort
from .._native import STATUS_MESSAGES, status_message
from ..core.error import SMRTError
from ..core.globalconstants import C_SPEED
from ..core.result import LabeledArray
from .dort import DORT, _Solution as _DortSolution


# ---- options ---------------------------------------------------------------------------------------------------------------
def check_error_handling(error_handling):
    if error_handling not in ("exception", "nan"):
        raise SMRTError("error_handling must be 'exception' or 'nan'")
    return error_handling


def positive_integer(value, what):
    """`value` as an int, refused unless it is a whole number >= 1 (a bool is none)."""
    try:
        whole = not isinstance(value, bool) and int(value) == value and value >= 1
    except (TypeError, ValueError):
        whole = False
    if not whole:
        raise SMRTError(what + " must be a positive integer")
    return int(value)


# ---- the group loop --------------------------------------------------------------------------------------------------------
class Group(types.SimpleNamespace):
    """One homogeneous group of a run, as the hooks of SolverBase see it:

    sel          indices of its simulations, in the order of the rows of its output
    u_packs      indices of its distinct snowpacks, ascending; u_freq: its distinct frequencies, ascending
    sensor0      its first sensor (what is uniform in the group is read from it)
    given, sps   its snowpacks as the caller gave them and as they are packed (_snowpack_key may replace them)
    names        the emmodel names of `sps`; sensor_of: {frequency: sensor}
    packer       the DORT subclass that packs it; batch: the PackedBatch (set by _prepare_group)
    pair_of_row  the pair (frequency index x len(u_packs) + snowpack index) of every row
    pairs        None when the rows are the whole batch in its order, otherwise pair_of_row (set before _launch)

    _prepare_group may add what its _launch needs (extras, params, ...)."""


class SolverBase(object):
    """Hooks (the first four have no default):

    _check_sensor(sensor)            refuse a sensor the solver cannot serve
    _sensor_key(sensor)              what must be uniform inside one launch on the sensor's side
    _packer()                        the DORT subclass that packs the batches
    _launch(ctx, group)              the device call of a group, under the context lock: its output
    _snowpack_key(sp, on_host)       (snowpack as it is packed, key of what must be uniform on the snowpack's side) or refuse
    _prepare_group(ctx, group)       pack the group; a solver adds what it evaluates on the host before the launch
    _status_message(out, at, status) the text of the first bad status word
    _after_group(group, out)         e.g. collect what the warnings of the run need
    _solution(...)                   the _Solution of the run
    """

    NAME = None                      # in the messages
    ATMOSPHERE = "the {} solver can not handle atmosphere yet."
    CHECKS_SENSOR_FIRST = True       # solve and solve_plan check the sensors before anything else
    launches = 0                     # launches of the last solve: tests assert "one launch per group"
    launch_info = ()                 # per launch, where the library reports it: dict(chunks, reserved_bytes, over_budget, budget)

    # ---- the reference's protocol --------------------------------------------------------------------------------
    def solve(self, snowpack, emmodels, sensor, atmosphere=None, parallel_computation=None):
        """One (snowpack, sensor configuration); `emmodels`: the per-layer instances made by Model.prepare_emmodels --
        smrt_amd's, or any object with the reference's emmodel protocol."""
        from ..core.foreign import adopt_snowpack, entry_of_instance

        if self.CHECKS_SENSOR_FIRST:
            self._check_sensor(sensor)
        snowpack = adopt_snowpack(snowpack)
        self._refuse_atmosphere(snowpack, atmosphere)
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

        if self.CHECKS_SENSOR_FIRST:
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

    def _context(self):
        """The context of the solver's GPU, through the dort module at call time.  The seven solver modules keep this method
        under their own name for get_context: their CPU tests put a stand-in there."""
        return dort.get_context((self.devices or [None])[0])

    def _refuse_atmosphere(self, sp, atmosphere=None):
        if atmosphere is not None or sp.atmosphere is not None:
            raise SMRTError(self.ATMOSPHERE.format(self.NAME))

    # ---- grouping, packing, launching ----------------------------------------------------------------------------
    def _solve_indexed(self, sensors, packs, sens_idx, pack_idx, emmodel_names, packer=None):
        packer = packer or self._packer()
        sens_idx, pack_idx = np.asarray(sens_idx), np.asarray(pack_idx)
        sensor_keys, pack_keys = {}, {}
        s_code = np.empty(len(sensors), np.int64)
        for k, sensor in enumerate(sensors):
            self._check_sensor(sensor)
            s_code[k] = sensor_keys.setdefault(self._sensor_key(sensor), len(sensor_keys))
        p_code = np.empty(len(packs), np.int64)
        packed = []
        for k, sp in enumerate(packs):
            on_host = not isinstance(emmodel_names, str) and any(not isinstance(e, str) for e in emmodel_names[k])
            as_packed, key = self._snowpack_key(sp, on_host)
            carry_plan_facts(packer, sp, as_packed)
            packed.append(as_packed)
            p_code[k] = pack_keys.setdefault(key, len(pack_keys))
        freq = np.array([float(s.frequency) for s in sensors])
        code = s_code[sens_idx] * len(pack_keys) + p_code[pack_idx]
        sol = self._solution(sensors, packs, sens_idx, pack_idx)
        ctx = self._context()
        self.launches, self.launch_info = 0, []
        for c in np.unique(code):
            sel = np.nonzero(code == c)[0]
            u_packs, inv_p = np.unique(pack_idx[sel], return_inverse=True)
            u_freq, inv_f = np.unique(freq[sens_idx[sel]], return_inverse=True)
            g = Group(sel=sel, u_packs=u_packs, u_freq=u_freq, sensor0=sensors[sens_idx[sel[0]]],
                      given=[packs[k] for k in u_packs], sps=[packed[k] for k in u_packs],
                      names=emmodel_names if isinstance(emmodel_names, str) else [emmodel_names[k] for k in u_packs],
                      sensor_of={float(sensors[k].frequency): sensors[k] for k in sens_idx[sel]},
                      packer=packer, batch=None, pair_of_row=inv_f * len(u_packs) + inv_p, pairs=None)
            self._prepare_group(ctx, g)
            n_pairs = g.batch.n_pairs
            full = len(g.pair_of_row) == n_pairs and np.array_equal(g.pair_of_row, np.arange(n_pairs))
            g.pairs = None if full else g.pair_of_row
            with ctx.lock:
                out = self._launch(ctx, g)
            self.launches += 1
            bad = np.argwhere(out.status != 0)
            if len(bad) and self.error_handling == "exception":
                at = tuple(bad[0])
                status = int(out.status[at])   # (status 5 on a Choudhury substrate names the validity range of the model)
                raise SMRTError(status_message(g.batch, status, self._status_message(out, at, status)))
            sol.add_group(sel, out, g.sps[0], (u_packs, np.array(g.batch.n_layers, np.int64), np.array(g.batch.thickness, float)))
            self._after_group(g, out)
        return sol

    def _snowpack_key(self, sp, on_host):
        self._refuse_atmosphere(sp)
        return sp, on_host

    def _prepare_group(self, ctx, g):
        g.batch = g.packer._pack(g.sensor0, g.sps, g.u_freq, g.names, g.sensor_of)

    def _status_message(self, out, at, status):
        return STATUS_MESSAGES.get(status, f"the {self.NAME} solver failed with status {status}")

    def _after_group(self, g, out):
        pass

    def _solution(self, sensors, packs, sens_idx, pack_idx):
        return _DortSolution(self, sensors, packs, sens_idx, pack_idx)


def carry_plan_facts(packer, sp, replacement):
    """A snowpack made for the packing alone answers with the layer facts of the snowpack of the plan it stands for."""
    if replacement is not sp and packer._plan_facts is not None:
        packer._plan_facts[id(replacement)] = packer._plan_facts.get(id(sp))


class RefusingPacker(DORT):
    """DORT's packing of layers and kinds for a solver that evaluates nothing on the host: everything DORT would evaluate
    there is refused, with the solver's own words."""

    SUBSTRATES_ON_HOST = INTERFACES_ON_HOST = IBA_SCALARS_ON_HOST = EVALUATE_ON_HOST = None

    def _substrates_on_host(self, *args, **kwargs):
        raise SMRTError(self.SUBSTRATES_ON_HOST)

    def _interfaces_on_host(self, *args, **kwargs):
        raise SMRTError(self.INTERFACES_ON_HOST)

    def _iba_scalars_on_host(self, *args, **kwargs):
        raise SMRTError(self.IBA_SCALARS_ON_HOST)

    def _evaluate_on_host(self, *args, **kwargs):
        raise SMRTError(self.EVALUATE_ON_HOST)


# ---- results ---------------------------------------------------------------------------------------------------------------
class LayeredSolution(_DortSolution):
    """dort._Solution for the solvers whose Result.other_data is made of the layer scalars alone: effective_permittivity, ks,
    ke, ka, the columns named in LAYER_EXTRA (from column 4 of the layer rows on) and the thickness -- per simulation with the
    layers as they were solved, stacked with NaN below the last layer of a shallower snowpack."""

    LAYER_EXTRA = ()

    def _layer_other(self, lay, thickness, wrap):
        other = {"effective_permittivity": wrap(lay[..., 0] + 1j * lay[..., 1], None), "ks": wrap(lay[..., 2], "ks"),
                 "ke": wrap(lay[..., 2] + lay[..., 3], "ke"), "ka": wrap(lay[..., 3], "ka")}
        for column, name in enumerate(self.LAYER_EXTRA, 4):
            other[name] = wrap(lay[..., column], name)
        other["thickness"] = wrap(thickness, "thickness")
        return other

    def _slot(self, group, pack_idx):
        """The row(s) of snowpack(s) `pack_idx` in the batch of a group."""
        return np.searchsorted(self.columns[group][0], pack_idx)

    def _other(self, i, labelled=LabeledArray):
        """(other_data of simulation i, its number of layers as solved)."""
        group = self.group_of[i]
        L = int(self.columns[group][1][self._slot(group, self.pack_idx[i])])
        layer_idx = ("layer", np.arange(L))
        thickness = np.asarray(self.packs[self.pack_idx[i]].layer_thicknesses, float)[:L]
        lay = self.outputs[group].layers[self.row_of[i]][:L]
        return self._layer_other(lay, thickness, lambda v, name: labelled(v.copy(), [layer_idx], name=name)), L

    def _grid(self, plan):
        """(first sensor, leading coordinates, their shape) when the simulations are one homogeneous grid of the plan's dimensions
        -- one device group, one channel map -- otherwise None: the caller then nests per-simulation results."""
        if len(self.outputs) != 1 or not plan.dimensions:
            return None
        sensor0 = self.sensors[0]
        if any(s.channel_map != sensor0.channel_map for s in self.sensors[1:]):
            return None
        lead = [(name, np.asarray(list(values))) for name, values in plan.dimensions]
        shape = tuple(len(v) for _, v in lead)
        if int(np.prod(shape)) != len(self.row_of):
            return None
        return sensor0, lead, shape

    def _stacked_layers(self, lead, shape):
        """(other_data of the stacked result, layers solved per simulation, the largest of them)."""
        out, order = self.outputs[0], self.row_of
        u_packs, nl_solved, thick_solved = self.columns[0]
        slot = self._slot(0, self.pack_idx)
        nl = nl_solved[slot]
        Lmax = int(nl.max())
        lay = out.layers[order][:, :Lmax].copy()
        below = np.arange(Lmax)[None, :] >= nl[:, None]
        lay[below] = np.nan
        thick = thick_solved.reshape(len(u_packs), -1)[slot, :Lmax].copy()
        thick[below] = np.nan
        layer_dim = [("layer", np.arange(Lmax))]

        def stack(v, name):
            return LabeledArray(v.reshape(shape + (Lmax,)), lead + layer_dim, name=name)

        return self._layer_other(lay, thick, stack), nl, Lmax


# ---- what the altimetry solvers evaluate on the host in the same way ---------------------------------------------------------
def layer_permittivities(ctx, batch, packer, params):
    """[n_pairs, Lmax, 2]: real and imaginary part of the effective permittivity of every layer of a packed group -- the
    caller's own when its emmodels were evaluated on the host (batch.host_layer), otherwise the device's: the (pair, layer)
    kernel alone (DortContext.lrm_layers with `params`), not a launch of the solver."""
    Lmax = int(batch.struct.n_layers_max)
    if packer.host_emmodels is not None:
        return batch.host_layer.reshape(-1, Lmax, 4)[..., 2:4]
    with ctx.lock:
        return np.asarray(ctx.lrm_layers(batch, params)).reshape(-1, Lmax, 5)[..., 0:2]


def coherent_factor(sensor, wavenumber, roughness_rms, mu):
    """What Flat's specular reflection is multiplied with for the coherent echo of a spherical wave on a boundary of
    roughness_rms, seen under the cosine(s) mu (Fung and Eom 1983, eq. 6)."""
    beta0 = np.sqrt(C_SPEED / (sensor.pulse_bandwidth * sensor.altitude)) * np.sqrt(2)
    beta12 = 1 / (wavenumber * sensor.altitude * beta0) ** 2 + beta0 ** 2 / 4
    return np.exp(-4 * (wavenumber * roughness_rms) ** 2 - (1 - mu ** 2) / beta12) / beta12 / (4 * np.pi)
