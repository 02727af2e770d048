"""Nadir LRM altimetry solver, MI355X-native (drop-in for smrt/rtsolver/nadir_lrm_altimetry.py).

The waveform a low-rate-mode radar altimeter (ENVISAT RA-2, SARAL / AltiKa, Sentinel-3 in LRM, ...) measures over a layered
snowpack (Adams and Brown 1998; Lacroix et al. 2008; Larue et al. 2021): first order scattering, paths along the vertical, the
vertical distribution of the volume, interface and surface echo convolved with Brown's flat surface impulse response.

    from smrt_amd.inputs import lrm_altimeter_list
    m = make_model("iba", "nadir_lrm_altimetry", rtsolver_options={"return_contributions": True})
    res = m.run(lrm_altimeter_list.envisat_ra2("Ku"), snowpacks)
    res.waveform(contribution="volume"), res.delay, res.gate, res.z_gate

The result has the dimensions (delay, theta_inc, theta), `contribution` (surface, interfaces, volume, total) in front with
return_contributions.  `snowpack.sigma_surface` (m) and `snowpack.surface_slope` (degrees) are read when set.

The arithmetic runs in three HIP kernels through the C ABI (include/smrt_dort.h: smrt_lrm_*); packing of layers and kinds is
DORT's.  Flat and Transparent interfaces are evaluated on the device; any other interface or substrate object is evaluated here,
per incidence sample, through the reference's protocol and handed over as numbers.  A whole Model.run is one launch per group
(same sensor configuration, same options, same number of incidence samples).

Refused, because the reference itself cannot run them: theta_inc_sampling > 1 with sigma_surface > 0; the
coherent reflection of an interface whose roughness_rms is None; theta_inc_sampling = 1 with the coherent reflection on a
snowpack that mixes interfaces with and without roughness_rms; any waveform model but Brown1977; skip_pfs_convolution with
theta_inc_sampling > 1; pitch / roll together with a surface slope.
"""
import numpy as np

from .._native import STATUS_MESSAGES, PackedLrmParams
from ..core.error import SMRTError
from ..core.globalconstants import C_SPEED
from ..core.result import AltimetryResult, LabeledArray
from ..core.sensor import Altimeter
from ..interface.flat import Flat
from ..interface.fresnel import reflection_diagonal
from ..interface.transparent import Transparent
from .dort import DORT, get_context
from .iterative_first_order import IterativeFirstOrder, _Packer
from .lrm_waveform_model import Brown1977  # noqa: F401  (waveform_model=Brown1977)

CONTRIBUTIONS = ["surface", "interfaces", "volume", "total"]


class NadirLRMAltimetry(object):
    """Options as smrt/rtsolver/nadir_lrm_altimetry.py; `devices` (list of GPU indices; the first is used) is smrt_amd's own."""

    _broadcast_capability = {}

    def __init__(self, waveform_model=None, oversampling_time=10, return_oversampled=False, skip_pfs_convolution=False,
                 return_contributions=False, compute_coherent_reflection=True, theta_inc_sampling=8, error_handling="exception",
                 devices=None):
        if error_handling not in ("exception", "nan"):
            raise SMRTError("error_handling must be 'exception' or 'nan'")
        if waveform_model is not None and getattr(waveform_model, "__name__", "") not in ("Brown1977", "brown_1977"):
            raise SMRTError("the nadir_lrm_altimetry solver offers the Brown1977 waveform model only (a model without an "
                            "analytical PFS cannot run in the reference either)")
        if isinstance(oversampling_time, bool) or int(oversampling_time) != oversampling_time or oversampling_time < 1:
            raise SMRTError("oversampling_time must be a positive integer")
        if isinstance(theta_inc_sampling, bool) or int(theta_inc_sampling) != theta_inc_sampling or theta_inc_sampling < 1:
            raise SMRTError("theta_inc_sampling must be a positive integer")
        if skip_pfs_convolution and theta_inc_sampling > 1:
            raise SMRTError("skip_pfs_convolution is offered with theta_inc_sampling=1 only (the reference returns an array "
                            "that does not fit its coordinates otherwise)")
        self.error_handling = error_handling
        self.oversampling = int(oversampling_time)
        self.return_oversampled, self.skip_pfs_convolution = bool(return_oversampled), bool(skip_pfs_convolution)
        self.return_contributions = bool(return_contributions)
        self.compute_coherent_reflection = bool(compute_coherent_reflection)
        self.theta_inc_sampling = int(theta_inc_sampling)
        self.devices = devices
        self.launches = 0   # launches of the last solve: tests assert "one launch per group"

    # ---- the reference's protocol --------------------------------------------------------------------------------
    def solve(self, snowpack, emmodels, sensor, atmosphere=None, parallel_computation=None):
        from ..core.foreign import adopt_snowpack, entry_of_instance

        snowpack = adopt_snowpack(snowpack)
        if atmosphere is not None:
            raise SMRTError("the nadir_lrm_altimetry solver can not handle atmosphere.")
        if len(emmodels) != snowpack.nlayer:
            raise SMRTError("one emmodel per layer is needed")
        entries = [entry_of_instance(e, layer) for e, layer in zip(emmodels, snowpack.layers)]
        return self.solve_batch([(sensor, snowpack)], [entries])[0]

    solve_batch = IterativeFirstOrder.solve_batch
    emmodel_names = DORT.emmodel_names

    def solve_plan(self, model, plan):
        """The whole plan of a Model.run, packed once and launched once per group."""
        from ..core.model import nest_results

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

    # ---- checks ------------------------------------------------------------------------------------------------------
    def _check_sensor(self, sensor):
        if not isinstance(sensor, Altimeter) and not hasattr(sensor, "pulse_bandwidth"):
            raise SMRTError("the nadir_lrm_altimetry solver needs an altimeter sensor (smrt_amd.inputs.lrm_altimeter_list)")
        if np.ndim(sensor.frequency) != 0:
            raise SMRTError("the nadir_lrm_altimetry solver does not broadcast the frequency: split the sensor first (Model.run does)")
        if np.any(np.asarray(sensor.theta_inc) != 0):
            raise SMRTError("This solver is for nadir looking altimeter only")
        if self.theta_inc_sampling == 1 and not self.skip_pfs_convolution:
            # the reference shifts the impulse response to the first sub-gate at or after the nominal gate and fails when there
            # is none, or when it is the first one (lrm_waveform_model.py: PFS_PTR_PDF)
            t_gate = np.arange(0, sensor.ngate * self.oversampling) / (sensor.pulse_bandwidth * self.oversampling)
            shift = int((t_gate - sensor.nominal_gate / sensor.pulse_bandwidth >= 0).argmax())
            if shift < 1:
                raise SMRTError("the nominal gate must lie inside the gate window, after its first sub-gate (0 < nominal_gate "
                                "< ngate): the reference cannot shift the impulse response otherwise")
        if self.theta_inc_sampling > 1 and sensor.ngate % self.theta_inc_sampling != 0:
            raise SMRTError("The number 'theta_inc_sampling' must be a true divider of the number of gates.")

    def _check_snowpack(self, sp, sensor):
        if sp.atmosphere is not None:
            raise SMRTError("the nadir_lrm_altimetry solver can not handle atmosphere.")
        sigma, slope = float(getattr(sp, "sigma_surface", 0) or 0), float(getattr(sp, "surface_slope", 0) or 0)
        if self.theta_inc_sampling > 1 and sigma > 0:
            raise SMRTError("theta_inc_sampling > 1 can not be combined with sigma_surface > 0 (the reference reads a pulse_sigma "
                            "the altimeter does not have): use theta_inc_sampling=1")
        if slope != 0 and sensor.off_nadir_angle != 0:
            raise SMRTError("It is currently not possible to account for both off_nadir and tilted terrain.")
        if self.compute_coherent_reflection:
            objs = list(sp.interfaces) + ([sp.substrate] if sp.substrate is not None else [])
            has = [hasattr(o, "roughness_rms") for o in objs]
            if any(h and o.roughness_rms is None for h, o in zip(has, objs)):
                raise SMRTError("the coherent reflection needs the roughness_rms of every rough interface and substrate: one is "
                                "None (set roughness_rms, or compute_coherent_reflection=False)")
            if self.theta_inc_sampling == 1 and any(has) and not all(has):
                raise SMRTError("with theta_inc_sampling=1 the coherent reflection needs interfaces (and a substrate) that all have a "
                                "roughness_rms or all have none (the reference fails on the mixture): use theta_inc_sampling > 1 "
                                "or compute_coherent_reflection=False")
        return sigma, np.deg2rad(slope)

    def _packer(self):
        return _Packer(n_max_stream=2, m_max=0, error_handling=self.error_handling, devices=self.devices)

    def _t_inc(self, sensor):
        if self.theta_inc_sampling > 1:
            return np.linspace(0, sensor.ngate / sensor.pulse_bandwidth, self.theta_inc_sampling + 1)
        return np.zeros(1)

    # ---- grouping, packing, launching ----------------------------------------------------------------------------
    def _solve_indexed(self, sensors, packs, sens_idx, pack_idx, emmodel_names, packer=None):
        packer = packer or self._packer()
        keys = {}
        s_code = np.empty(len(sensors), np.int64)
        for k, sensor in enumerate(sensors):
            self._check_sensor(sensor)
            key = tuple(float(getattr(sensor, a)) for a in ("altitude", "pulse_bandwidth", "beamwidth_alongtrack", "beamwidth_acrosstrack",
                                                            "antenna_gain", "ngate", "nominal_gate", "pitch_angle", "roll_angle"))
            s_code[k] = keys.setdefault(key, len(keys))
        on_host = np.array([not isinstance(emmodel_names, str) and any(not isinstance(e, str) for e in emmodel_names[k])
                            for k in range(len(packs))], np.int64)
        freq = np.array([float(s.frequency) for s in sensors])
        code = s_code[sens_idx] * 2 + on_host[pack_idx]
        sol = _Solution(self, sensors, packs, sens_idx, pack_idx)
        ctx = get_context((self.devices or [None])[0])
        self.launches = 0
        for g in np.unique(code):
            sel = np.nonzero(code == g)[0]
            u_packs, inv_p = np.unique(pack_idx[sel], return_inverse=True)
            u_freq, inv_f = np.unique(freq[sens_idx[sel]], return_inverse=True)
            sensor0 = sensors[sens_idx[sel[0]]]
            sps = [packs[k] for k in u_packs]
            surf = np.array([self._check_snowpack(sp, sensor0) for sp in sps])
            names = emmodel_names if isinstance(emmodel_names, str) else [emmodel_names[k] for k in u_packs]
            sensor_of = {float(sensors[k].frequency): sensors[k] for k in sens_idx[sel]}
            packer.host_emmodels = None
            bare = [sp if sp.substrate is None else _without_substrate(sp, packer) for sp in sps]
            batch = packer._pack(sensor0, bare, u_freq, names, sensor_of)
            t_inc = self._t_inc(sensor0)
            options = dict(oversampling=self.oversampling, t_inc=t_inc, return_contributions=self.return_contributions,
                           return_oversampled=self.return_oversampled, skip_pfs_convolution=self.skip_pfs_convolution,
                           sigma_surface=surf[:, 0] if surf[:, 0].any() else None, surface_slope=surf[:, 1] if surf[:, 1].any() else None)
            itf = self._interface_values(ctx, batch, packer, sensor0, sps, u_freq, t_inc, options)
            params = PackedLrmParams(sensor0, interface_values=itf, **options)
            pairs = inv_f * len(u_packs) + inv_p
            full = len(pairs) == batch.n_pairs and np.array_equal(pairs, np.arange(batch.n_pairs))
            with ctx.lock:
                out = ctx.lrm_run(batch, params, pairs=None if full else pairs)
            self.launches += 1
            bad = np.nonzero(out.status != 0)[0]
            if len(bad) and self.error_handling == "exception":
                st = int(out.status[bad[0]])
                raise SMRTError(STATUS_MESSAGES.get(st, f"the nadir_lrm_altimetry solver failed with status {st}"))
            sol.add_group(sel, out, (u_packs, np.array(batch.n_layers, np.int64), np.array(batch.thickness, float)))
        return sol

    # ---- what the host evaluates (include/smrt_dort.h: smrt_lrm_params.interface_values) ----------------------------
    def _interface_values(self, ctx, batch, packer, sensor0, sps, freqs, t_inc, options):
        """[F, S, Lmax + 1, 1 + n_mu] or None when every interface is Flat and there is no substrate: the one-way transmission at
        nadir (NaN: Flat, -1: Transparent, both on the device) and the echo per incidence sample of every boundary."""
        def on_device(itf):
            return isinstance(itf, (Flat, Transparent))

        if all(on_device(i) for sp in sps for i in sp.interfaces) and all(sp.substrate is None for sp in sps):
            return None
        F, S, Lmax, n_mu = len(freqs), len(sps), int(batch.struct.n_layers_max), len(t_inc)
        if packer.host_emmodels is not None:
            eps = batch.host_layer.reshape(F, S, Lmax, 4)[..., 2]
        else:   # the device's own permittivities: the (pair, layer) kernel alone, not a launch of the solver
            with ctx.lock:
                layers = ctx.lrm_layers(batch, PackedLrmParams(sensor0, **dict(options, sigma_surface=None, surface_slope=None)))
            eps = np.asarray(layers).reshape(F, S, Lmax, 5)[..., 0]
        mu_i = 1.0 / (1.0 + C_SPEED * t_inc / sensor0.altitude) if n_mu > 1 else np.ones(1)
        mu_i = mu_i * np.cos(sensor0.pitch_angle) * np.cos(sensor0.roll_angle)
        values = np.zeros((F, S, Lmax + 1, 1 + n_mu))
        values[..., 0] = np.nan
        for fi, f in enumerate(freqs):
            wavenumber = 2 * np.pi * float(f) / C_SPEED
            for s, sp in enumerate(sps):
                L = sp.nlayer
                e = np.concatenate([[1.0], eps[fi, s, :L]])
                for k, itf in enumerate(sp.interfaces):
                    if isinstance(itf, Transparent):
                        values[fi, s, k, 0] = -1.0
                    if on_device(itf):
                        continue
                    mu = np.sqrt(1 - (1 - mu_i) / e[k]).real
                    t = itf.coherent_transmission_matrix(float(f), e[k], e[k + 1], np.ones(1), 2)
                    values[fi, s, k, 0] = IterativeFirstOrder._rows(t, 1)[0, 0]
                    values[fi, s, k, 1:] = self._echo(itf, sensor0, wavenumber, float(f), e[k], e[k + 1], mu, False)
                if sp.substrate is not None:
                    mu = np.sqrt(1 - (1 - mu_i) / e[L]).real
                    values[fi, s, L, 1:] = self._echo(sp.substrate, sensor0, wavenumber, float(f), e[L], None, mu, True)
        return values

    def _echo(self, obj, sensor, wavenumber, frequency, eps_1, eps_2, mu, substrate):
        """Diffuse backscatter at (mu, mu, pi) divided by eps_1 (the refraction of the upwelling stream) plus, for an object with
        a roughness_rms, Flat's specular reflection times the coherent factor of a spherical wave (Fung and Eom 1983, eq. 6)."""
        n = len(mu)
        args = (frequency, eps_1) if substrate else (frequency, eps_1, eps_2)
        echo = np.zeros(n)
        if callable(getattr(obj, "diffuse_reflection_matrix", None)):
            echo = IterativeFirstOrder._dense(obj.diffuse_reflection_matrix(*args, mu, mu, np.pi, 2), n)[:, 0, 0] / eps_1
        if self.compute_coherent_reflection and hasattr(obj, "roughness_rms"):
            below = complex(obj.permittivity(frequency)) if substrate else eps_2
            specular = np.asarray(reflection_diagonal(eps_1, below, mu, 2), float)[0]
            beta0 = np.sqrt(C_SPEED / (sensor.pulse_bandwidth * sensor.altitude)) * np.sqrt(2)
            beta12 = 1 / (wavenumber * sensor.altitude * beta0) ** 2 + beta0 ** 2 / 4
            factor = np.exp(-4 * (wavenumber * obj.roughness_rms) ** 2 - (1 - mu ** 2) / beta12) / beta12 / (4 * np.pi)
            echo = echo + specular * factor
        return echo


def _without_substrate(sp, packer):
    """The snowpack as DORT's packer sees it here: the substrate enters through the interface values, not through the batch."""
    from ..core.snowpack import Snowpack

    bare = Snowpack(layers=sp.layers, interfaces=[Flat() for _ in sp.layers])
    if packer._plan_facts is not None:
        packer._plan_facts[id(bare)] = packer._plan_facts.get(id(sp))
    return bare


class _Solution:
    """Outputs of the device batches of one call, addressable per simulation and stackable as one result."""

    def __init__(self, solver, sensors, packs, sens_idx, pack_idx):
        self.solver, self.sensors, self.packs = solver, sensors, packs
        self.sens_idx, self.pack_idx = np.asarray(sens_idx), np.asarray(pack_idx)
        n = len(self.sens_idx)
        self.group_of, self.row_of = np.full(n, -1, np.int64), np.zeros(n, np.int64)
        self.outputs, self.columns = [], []

    def add_group(self, sel, out, columns):
        self.group_of[sel] = len(self.outputs)
        self.row_of[sel] = np.arange(len(sel))
        self.outputs.append(out)
        self.columns.append(columns)

    def _delay(self, sensor):
        so = self.solver
        t_gate = np.arange(0, sensor.ngate * so.oversampling) / (sensor.pulse_bandwidth * so.oversampling)
        if so.oversampling > 1 and not so.return_oversampled:
            t_gate = t_gate[::so.oversampling]
        return t_gate - sensor.nominal_gate / sensor.pulse_bandwidth

    def _coords(self, sensor):
        coords = [("delay", self._delay(sensor)), ("theta_inc", [0]), ("theta", [0])]
        return ([("contribution", CONTRIBUTIONS)] if self.solver.return_contributions else []) + coords

    def _values(self, values):
        """[..., rows, n] -> [..., n, 1, 1], or [..., 4, n, 1, 1] with the total last."""
        if self.solver.return_contributions:
            values = np.concatenate([values, np.sum(values, axis=-2)[..., None, :]], axis=-2)
        else:
            values = values[..., 0, :]
        return values[..., None, None]

    @staticmethod
    def _attrs(sensor):
        return dict(pulse_bandwidth=float(sensor.pulse_bandwidth), nominal_gate=float(sensor.nominal_gate))

    def _result(self, sensor, data, z_gate, other):
        data.attrs.update(self._attrs(sensor))
        return AltimetryResult(data, channel_map=sensor.channel_map, other_data=other, z_gate=z_gate)

    @staticmethod
    def _foreign(sensor):
        """(AltimetryResult, labelled-array constructor) of the package a foreign sensor belongs to -- the reference's own
        result over xarray, so that its concat_results nests what its Model.run gets back -- or None for smrt_amd's."""
        import importlib

        from ..core.foreign import NATIVE, package_of, result_factory

        root = package_of(sensor)
        if root == NATIVE:
            return None
        make, labelled = result_factory(sensor)
        if labelled is LabeledArray:
            return None
        cls = getattr(importlib.import_module(root + ".core.result"), "AltimetryResult", None)
        return (cls, labelled) if cls is not None else None

    def result(self, i):
        sensor, sp = self.sensors[self.sens_idx[i]], self.packs[self.pack_idx[i]]
        out, row = self.outputs[self.group_of[i]], self.row_of[i]
        L = sp.nlayer
        lay = out.layers[row][:L]
        layer_idx = ("layer", np.arange(L))
        other = {
            "effective_permittivity": LabeledArray(lay[:, 0] + 1j * lay[:, 1], [layer_idx]),
            "ks": LabeledArray(lay[:, 2].copy(), [layer_idx], name="ks"),
            "ke": LabeledArray(lay[:, 2] + lay[:, 3], [layer_idx], name="ke"),
            "ka": LabeledArray(lay[:, 3].copy(), [layer_idx], name="ka"),
            "backward_scattering": LabeledArray(lay[:, 4].copy(), [layer_idx], name="backward_scattering"),
            "thickness": LabeledArray(np.asarray(sp.layer_thicknesses, float), [layer_idx], name="thickness"),
        }
        coords = self._coords(sensor)
        foreign = self._foreign(sensor)
        if foreign is not None:   # as the reference builds it: the gate as a coordinate of delay where xarray can, z_gate an attribute
            cls, labelled = foreign
            data = labelled(self._values(out.values[row]), coords)
            if hasattr(data, "assign_coords"):
                data = data.assign_coords(gate=("delay", coords[-3][1] * sensor.pulse_bandwidth + sensor.nominal_gate))
            res = cls(data, channel_map=sensor.channel_map,
                      other_data={k: labelled(v.values, list(v.coords.items()), name=v.name) for k, v in other.items()})
            res.z_gate = labelled(out.z_gate[row].copy(), [coords[-3]], name="z_gate")
            return res
        z_gate = LabeledArray(out.z_gate[row].copy(), [coords[-3]], name="z_gate")
        return self._result(sensor, LabeledArray(self._values(out.values[row]), coords), z_gate, other)

    def stacked_result(self, plan):
        if len(self.outputs) != 1 or not plan.dimensions:
            return None
        sensor0 = self.sensors[0]
        if any(s.channel_map != sensor0.channel_map for s in self.sensors[1:]) or self._foreign(sensor0) is not None:
            return None
        out, order = self.outputs[0], self.row_of
        lead = [(name, np.asarray(list(values))) for name, values in plan.dimensions]
        shape = tuple(len(v) for _, v in lead)
        if int(np.prod(shape)) != len(order):
            return None
        values = self._values(out.values[order])
        coords = self._coords(sensor0)
        data = LabeledArray(values.reshape(shape + values.shape[1:]), lead + coords)
        z_gate = LabeledArray(out.z_gate[order].reshape(shape + (-1,)), lead + [coords[-3]], name="z_gate")
        u_packs, nl_solved, thick_solved = self.columns[0]
        slot = np.full(len(self.packs), -1, np.int64)
        slot[u_packs] = np.arange(len(u_packs))
        nl = nl_solved[slot[self.pack_idx]]
        Lmax = int(nl.max())
        lay = out.layers[order][:, :Lmax].copy()
        below = np.arange(Lmax)[None, :] >= nl[:, None]
        lay[below] = np.nan
        thick = thick_solved.reshape(len(u_packs), -1)[slot[self.pack_idx], :Lmax].copy()
        thick[below] = np.nan
        layer_dim = [("layer", np.arange(Lmax))]

        def stack(v, name=None):
            return LabeledArray(v.reshape(shape + (Lmax,)), lead + layer_dim, name=name)

        other = {
            "effective_permittivity": stack(lay[:, :, 0] + 1j * lay[:, :, 1]),
            "ks": stack(lay[:, :, 2], "ks"), "ke": stack(lay[:, :, 2] + lay[:, :, 3], "ke"), "ka": stack(lay[:, :, 3], "ka"),
            "backward_scattering": stack(lay[:, :, 4], "backward_scattering"), "thickness": stack(thick, "thickness"),
        }
        return self._result(sensor0, data, z_gate, other)
