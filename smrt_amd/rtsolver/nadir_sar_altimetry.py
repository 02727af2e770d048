"""Nadir SAR altimetry solver, MI355X-native (drop-in for smrt/rtsolver/nadir_sar_altimetry.py with its default delay-Doppler
model, Dinardo et al. 2018).

The delay-Doppler map a SAR-mode radar altimeter (CryoSat-2, Sentinel-3, CRISTAL) measures over a layered snowpack (Picard et al.
2025; Larue et al. 2021): first order scattering, paths along the vertical, the volume backscatter per sub-gate convolved along the
delay with the map of a surface of constant backscatter, the echo of the surface and of every interface as that map at the
boundary's own mean square slope, shifted to the boundary's two-way travel time.

    from smrt_amd.core.terrain import TerrainInfo
    from smrt_amd.inputs import sar_altimeter_list
    sp.terrain_info = TerrainInfo(sigma_surface=0.2)
    m = make_model("iba", "nadir_sar_altimetry", rtsolver_options={"return_contributions": "basic coherent"})
    res = m.run(sar_altimeter_list.cryosat2_sarm(), snowpacks)
    res.delay_doppler_map(contribution="volume"), res.waveform(), res.z_gate, res.doppler_frequency, res.doppler_bin

The result has the dimensions (delay, doppler_frequency, theta_inc, theta), `contribution` in front with return_contributions.

The arithmetic runs in four HIP kernels through the C ABI (include/smrt_dort.h: smrt_sar_*); packing of layers and kinds is DORT's.
Every interface and the substrate is evaluated here at nadir through the reference's protocol and handed over as numbers.  A whole
Model.run is one launch per group (same sensor, same options), unless the maps of a group and the f0 / f1 tables of its distinct
sigma_surface exceed OUTPUT_BUDGET bytes: the pairs of the group are then launched in as many parts as needed, each with the
tables of its own sigma_surface only.

delay_doppler_model="halimi14" (Halimi et al. 2014) takes ptr_time / ptr_doppler (None or "sinc^2"),
slant_range_correction and delay_window_widening in delay_doppler_model_options: one table per distinct sigma_surface, made on the
device by direct convolution, for the volume and every boundary alike; no mean_square_slope is needed, and the coherent echo is
added after a warning, as in the reference.

Refused: any delay_doppler_model but Dinardo18 and Halimi14; theta_inc != 0; an atmosphere; an interface or substrate
without roughness_rms; with Dinardo18 a positive incoherent echo without mean_square_slope; skip_convolutions; a terrain that is not "normal"; an odd
ndoppler; a boundary with a positive echo later than the window.  Of smrt_amd's own: a dem or a slope_angle in the terrain_info.
"""
import numpy as np

from .._native import PackedLrmParams, PackedSarParams, ptr_gaussian_approximation
from ..core.error import SMRTError, smrt_warn
from ..core.globalconstants import C_SPEED
from ..core.sensor import Altimeter
from ..core.terrain import TerrainInfo
from ..interface.fresnel import reflection_diagonal
from .delay_doppler_model.dinardo18 import Dinardo18  # noqa: F401  (delay_doppler_model=Dinardo18)
from .delay_doppler_model.halimi14 import Halimi14  # noqa: F401  (delay_doppler_model=Halimi14)
from .dort import get_context
from .iterative_first_order import IterativeFirstOrder
from .nadir_lrm_altimetry import NadirLRMAltimetry, _Solution as _LrmSolution, _without_substrate
from .solver_base import SolverBase, check_error_handling, coherent_factor, layer_permittivities, positive_integer

OUTPUT_BUDGET = 1 << 30   # bytes of the maps and of the f0 / f1 tables of one launch


class NadirSARAltimetry(NadirLRMAltimetry):
    """Options as smrt/rtsolver/nadir_sar_altimetry.py; `devices` (list of GPU indices; the first is used) is smrt_amd's own."""

    _broadcast_capability = {}
    NAME = "nadir_sar_altimetry"

    def __init__(self, delay_doppler_model=None, delay_doppler_model_options=None, oversampling_time=4, oversampling_doppler=4,
                 return_oversampled=False, skip_convolutions=False, return_contributions=False, theta_inc_sampling=8,
                 error_handling="exception", prune_deep_snowpack=True, devices=None):
        check_error_handling(error_handling)
        name = delay_doppler_model if isinstance(delay_doppler_model, str) else getattr(delay_doppler_model, "__name__", None)
        model = "dinardo18" if delay_doppler_model is None else (name or "").lower()
        if model not in ("dinardo18", "halimi14"):
            raise SMRTError("the nadir_sar_altimetry solver offers the Dinardo18 and the Halimi14 delay Doppler models only (the "
                            "others rest on adaptive quadrature, FFT grids or a DEM)")
        self.delay_doppler_model = model
        options = dict(delay_doppler_model_options or {})
        self.ptr_doppler, self.slant_range_correction, self.delay_window_widening = "gaussian-smrt", True, 1
        if model == "halimi14":   # (the solver's own oversampling factors govern, as in the reference)
            unknown = set(options) - {"ptr_time", "ptr_doppler", "slant_range_correction", "delay_window_widening", "oversampling_time",
                                      "oversampling_doppler"}
            if unknown:
                raise SMRTError(f"Halimi14 has no option {sorted(unknown)}: it takes ptr_time, ptr_doppler, slant_range_correction and "
                                "delay_window_widening")
            for what in ("ptr_time", "ptr_doppler"):
                if options.get(what) not in (None, "sinc^2"):
                    raise SMRTError(f"Halimi14 takes {what}=None or 'sinc^2' only (as the reference, which raises NotImplementedError)")
            self.delay_window_widening = positive_integer(options.get("delay_window_widening", 1), "delay_window_widening")
            self.slant_range_correction = bool(options.get("slant_range_correction", True))
        else:
            unknown = set(options) - {"ptr_time", "ptr_doppler", "oversampling_time", "oversampling_doppler"}
            if unknown:
                raise SMRTError(f"Dinardo18 has no option {sorted(unknown)}: it takes ptr_time and ptr_doppler")
            if not (options.get("ptr_time") or "gaussian").startswith("gaussian"):
                raise SMRTError("Dinardo18 takes a Gaussian ptr_time only")
            self.ptr_doppler = options.get("ptr_doppler", "gaussian-smrt")
        self.oversampling_time = positive_integer(oversampling_time, "oversampling_time")
        self.oversampling_doppler = positive_integer(oversampling_doppler, "oversampling_doppler")
        if skip_convolutions:
            raise SMRTError("skip_convolutions is not implemented (nor in the reference)")
        if return_contributions is True:
            return_contributions = "basic"
        if not return_contributions:
            return_contributions = "no"
        if return_contributions not in ("no", "basic", "basic coherent", "full", "full coherent"):
            raise SMRTError('Invalid return_contributions. It must be None, "no", basic", "basic coherent", "full" or "full coherent"')
        self.return_coherent = return_contributions.endswith(" coherent")
        self.return_contributions = return_contributions.replace(" coherent", "")
        self.error_handling = error_handling
        self.return_oversampled, self.skip_convolutions = bool(return_oversampled), False
        self.theta_inc_sampling = theta_inc_sampling   # (the geometrical-optics branch evaluates nadir only)
        self.prune_deep_snowpack = bool(prune_deep_snowpack)
        self.devices = devices

    # ---- checks ------------------------------------------------------------------------------------------------------
    def _check_sensor(self, sensor):
        if not isinstance(sensor, Altimeter) and not hasattr(sensor, "pulse_repetition_frequency"):
            raise SMRTError("the nadir_sar_altimetry solver needs a SAR altimeter sensor (smrt_amd.inputs.sar_altimeter_list)")
        if np.ndim(sensor.frequency) != 0:
            raise SMRTError("the nadir_sar_altimetry solver does not broadcast the frequency: split the sensor first (Model.run does)")
        if np.any(np.asarray(sensor.theta_inc) != 0):
            raise SMRTError("This solver is for nadir looking altimeter only. Satellite mis-pointing (pitch and roll) is allowed.")
        if int(sensor.ndoppler) < 2 or int(sensor.ndoppler) % 2:
            raise SMRTError("the nadir_sar_altimetry solver needs an even, positive ndoppler (the reference's Doppler frequency "
                            "vector has another length than its map otherwise)")
        if not float(sensor.velocity) > 0 or not float(sensor.pulse_repetition_frequency) > 0:
            raise SMRTError("a SAR altimeter needs its velocity and its pulse_repetition_frequency")
        if self.delay_doppler_model == "dinardo18":
            ptr_gaussian_approximation(self.ptr_doppler, sensor.doppler_window)

    def _check_snowpack(self, sp, sensor=None):
        self._refuse_atmosphere(sp)
        info = getattr(sp, "terrain_info", None)
        info = TerrainInfo() if info is None else info
        model = "Halimi14" if self.delay_doppler_model == "halimi14" else "Dinardo18"
        if info.distribution != "normal":
            raise SMRTError(model + " is only available for a normally-distributed surface")
        if getattr(info, "dem", None) is not None or float(getattr(info, "slope_angle", 0) or 0) != 0:
            raise SMRTError(f"the nadir_sar_altimetry solver takes no dem and no slope_angle ({model} reads neither)")
        sigma = float(info.sigma_surface)
        if not sigma >= 0:
            raise SMRTError("terrain_info.sigma_surface must be non-negative")
        for obj in list(sp.interfaces) + ([sp.substrate] if sp.substrate is not None else []):
            if getattr(obj, "roughness_rms", None) is None:
                raise SMRTError("nadir_sar_altimetry only works with interfaces and substrates that define 'roughness_rms' to "
                                "compute the coherent reflection.")
        return sigma

    def _pruned(self, sp, sensor):
        """The snowpack the reference solves: without the layers below the depth the window reaches in vacuum, and then without
        the substrate."""
        if not self.prune_deep_snowpack:
            return sp
        depths = np.cumsum(sp.layer_thicknesses)
        reach = sensor.ngate / sensor.pulse_bandwidth * C_SPEED / 2
        if not depths[-1] > reach:
            return sp
        from ..core.snowpack import Snowpack

        n = int(np.searchsorted(depths, reach)) + 1
        if n >= sp.nlayer:
            return sp
        cut = Snowpack(layers=sp.layers[:n], interfaces=sp.interfaces[:n], terrain_info=getattr(sp, "terrain_info", None))
        cut.pruned_from = sp
        return cut

    def contributions(self, n_boundaries):
        """(names, row of every source: incoherent boundaries, coherent boundaries, volume; then the row of the total) for a
        snowpack of n_boundaries interfaces, the substrate counted when there is one.  As the reference: "full" without
        "coherent" has the incoherent echo alone in the row of an interface (the total has both)."""
        nb = n_boundaries
        if self.return_contributions == "no":
            return [], [-1] * (2 * nb + 1) + [0]
        if self.return_contributions == "basic":
            if self.return_coherent:
                names = ["incoherent surface", "coherent surface", "incoherent interfaces", "coherent interfaces", "volume", "total"]
                return names, [0] + [2] * (nb - 1) + [1] + [3] * (nb - 1) + [4, 5]
            return ["surface", "interfaces", "volume", "total"], ([0] + [1] * (nb - 1)) * 2 + [2, 3]
        if self.return_coherent:
            names = [f"incoherent interface {i}" for i in range(nb)] + [f"coherent interface {i}" for i in range(nb)] + ["volume", "total"]
            return names, list(range(2 * nb + 2))
        return [f"interface {i}" for i in range(nb)] + ["volume", "total"], list(range(nb)) + [-1] * nb + [nb, nb + 1]

    # ---- grouping, packing, launching ----------------------------------------------------------------------------
    def _sensor_key(self, sensor):
        return tuple(float(getattr(sensor, a)) for a in (
            "frequency", "altitude", "pulse_bandwidth", "beamwidth_alongtrack", "beamwidth_acrosstrack", "antenna_gain", "ngate",
            "ndoppler", "nominal_gate", "pitch_angle", "roll_angle", "velocity", "pulse_repetition_frequency")) + (
                sensor.doppler_window, self.delay_doppler_model, self.slant_range_correction, self.delay_window_widening)

    def _context(self):
        return get_context((self.devices or [None])[0])   # (this module's name: the CPU tests put a stand-in here)

    def _solution(self, sensors, packs, sens_idx, pack_idx):
        return _Solution(self, sensors, packs, sens_idx, pack_idx)

    def _prepare_group(self, ctx, g):
        """Packs the snowpacks the reference solves (_pruned) and evaluates their boundaries; sets g.sigma, g.values, g.row_map
        and g.n_rows for the launch."""
        sensor0, packer = g.sensor0, g.packer
        g.sigma = np.array([self._check_snowpack(sp) for sp in g.sps])
        g.sps = sps = [self._pruned(sp, sensor0) for sp in g.sps]
        if not isinstance(g.names, str):
            g.names = [list(names)[:sp.nlayer] for names, sp in zip(g.names, sps)]
        packer.host_emmodels = None
        bare = [_without_substrate(sp, packer) for sp in sps]
        for b, sp in zip(bare, sps):   # (a pruned snowpack is new to the plan: it has the facts of no snowpack of it)
            if packer._plan_facts is not None and packer._plan_facts.get(id(b)) is None:
                packer._plan_facts[id(b)] = b.layer_facts()
        g.batch = packer._pack(sensor0, bare, g.u_freq, g.names, g.sensor_of)   # (one frequency: it is part of the sensor key)
        Lmax = int(g.batch.struct.n_layers_max)
        g.values = self._boundary_values(ctx, g.batch, packer, sensor0, sps, Lmax)
        g.row_map = np.full((len(sps), 2 * (Lmax + 1) + 2), -1, np.int32)
        g.n_rows = 1
        for s, sp in enumerate(sps):
            nb = _n_boundaries(sp)
            names_s, rows = self.contributions(nb)
            g.row_map[s, :nb], g.row_map[s, Lmax + 1:Lmax + 1 + nb], g.row_map[s, -2:] = rows[:nb], rows[nb:2 * nb], rows[-2:]
            g.n_rows = max(g.n_rows, len(names_s), 1)

    def _launch(self, ctx, g):
        """The pairs of the group in as many parts as OUTPUT_BUDGET asks for, their outputs as one."""
        sensor0, sigma, n_rows = g.sensor0, g.sigma, g.n_rows
        pairs = np.asarray(g.pair_of_row, np.int64)
        # A part of the group holds its maps AND the tables of its own distinct sigma_surface (at worst one pair of tables
        # per snowpack) inside the budget.
        fine = sensor0.ngate * self.oversampling_time * sensor0.ndoppler * self.oversampling_doppler
        per_pair = n_rows * (fine if self.return_oversampled else sensor0.ngate * sensor0.ndoppler) * 8
        n_sigma = len(np.unique(sigma))
        # (Dinardo18: f0 and f1 per sigma_surface.  Halimi14: one table per sigma_surface, and once per launch the impulse
        # response convolved along Doppler on the widened window)
        halimi = self.delay_doppler_model == "halimi14"
        table, fixed = (fine * 8, fine * self.delay_window_widening * 8) if halimi else (2 * fine * 8, 0)
        step = max(1, (OUTPUT_BUDGET - fixed - min(n_sigma, len(pairs)) * table) // per_pair)
        if step < len(pairs):   # (several parts: each with at most `step` tables of its own)
            step = max(1, (OUTPUT_BUDGET - fixed) // (per_pair + table))
        outs = []
        for begin in range(0, len(pairs), step):
            part = pairs[begin:begin + step]
            full = len(part) == g.batch.n_pairs and np.array_equal(part, np.arange(g.batch.n_pairs))
            table_sigma, index = np.unique(sigma[part], return_inverse=True)
            table_index = np.zeros(len(g.sps), np.int32)      # (a snowpack outside the part is not read)
            table_index[part] = index
            params = PackedSarParams(sensor0, table_sigma, table_index, g.values, g.row_map, n_rows=n_rows,
                                     oversampling_time=self.oversampling_time, oversampling_doppler=self.oversampling_doppler,
                                     return_oversampled=self.return_oversampled, ptr_doppler=self.ptr_doppler,
                                     model=self.delay_doppler_model, slant_range_correction=self.slant_range_correction,
                                     delay_window_widening=self.delay_window_widening)
            outs.append(ctx.sar_run(g.batch, params, pairs=None if full else part))
        self.launches += len(outs) - 1   # (the group loop counts one)
        out = outs[0] if len(outs) == 1 else _joined(outs)
        out.n_boundaries = np.array([_n_boundaries(sp) for sp in g.sps], np.int64)   # (per snowpack of the batch, after pruning)
        return out

    def _status_message(self, out, at, status):
        if np.isfinite(out.echo[at]).all():
            return ("a boundary with a positive echo lies later than the window of the altimeter (the reference fails on "
                    "`0 <= itime < N`): use fewer layers, or a sensor with more gates")
        return SolverBase._status_message(self, out, at, status)

    # ---- what the host evaluates (include/smrt_dort.h: smrt_sar_params.boundary_values) ------------------------------
    def _boundary_values(self, ctx, batch, packer, sensor0, sps, Lmax):
        """[S, Lmax + 1, 4]: the one-way transmission at nadir, the coherent and the incoherent echo at the local incidence of the
        (mis-pointed) antenna, one over the mean square slope."""
        S, f = len(sps), float(sensor0.frequency)
        eps = layer_permittivities(ctx, batch, packer, None if packer.host_emmodels is not None else PackedLrmParams(sensor0))
        eps = eps[..., 0] + 1j * eps[..., 1]   # (the complex value: DESIGN.md 4h)
        mu_i = np.ones(1) * np.cos(sensor0.pitch_angle) * np.cos(sensor0.roll_angle)
        wavenumber = 2 * np.pi * f / C_SPEED
        values = np.zeros((S, Lmax + 1, 4))
        values[..., 0] = 1.0
        tabulated = self.delay_doppler_model == "halimi14"

        def echo(obj, e1, e2, mu, substrate):
            args = (f, e1) if substrate else (f, e1, e2)
            incoherent = 0.0
            if callable(getattr(obj, "diffuse_reflection_matrix", None)):
                incoherent = float(IterativeFirstOrder._dense(obj.diffuse_reflection_matrix(*args, mu, mu, np.pi, 2), 1)[0, 0, 0]) / e1.real
            below = complex(obj.permittivity(f)) if substrate else e2
            specular = float(np.asarray(reflection_diagonal(e1, below, mu, 2), float)[0, 0])
            coherent = specular * float(coherent_factor(sensor0, wavenumber, obj.roughness_rms, mu[0]))
            if tabulated:   # one map for the volume and every boundary: no mean square slope enters
                return coherent, incoherent, 0.0
            if incoherent > 0 and getattr(obj, "mean_square_slope", None) is None:
                raise SMRTError("the delay_doppler_model Dinardo18 relies on geometrical optics interfaces only (or non scattering "
                                "interfaces): an interface with an incoherent echo needs a mean_square_slope")
            return coherent, incoherent, (1.0 / float(obj.mean_square_slope) if incoherent > 0 else 0.0)

        for s, sp in enumerate(sps):
            L = sp.nlayer
            e = np.concatenate([[1.0 + 0j], eps[s, :L]])
            for k, itf in enumerate(sp.interfaces):
                mu = np.sqrt(1 - (1 - mu_i) / e[k]).real
                t = itf.coherent_transmission_matrix(f, e[k], e[k + 1], np.ones(1), 2)
                values[s, k, 0] = IterativeFirstOrder._rows(t, 1)[0, 0]
                values[s, k, 1:] = echo(itf, e[k], e[k + 1], mu, False)
            if sp.substrate is not None:
                mu = np.sqrt(1 - (1 - mu_i) / e[L].real)
                values[s, L, 1:] = echo(sp.substrate, e[L], None, mu, True)
        if tabulated and np.any(values[..., 1] > 0):   # (the reference adds it all the same, after this warning)
            smrt_warn("This delay Doppler model is not compatible with coherent backscatter")
        return values


def _n_boundaries(sp):
    return sp.nlayer + (sp.substrate is not None)


def _joined(outs):
    """The outputs of the parts of one group as one."""
    first = outs[0]
    for name in ("values", "status", "z_gate", "layers", "vertical", "echo"):
        setattr(first, name, np.concatenate([getattr(o, name) for o in outs]))
    return first


class _Solution(_LrmSolution):
    """Outputs of the device batches of one call, addressable per simulation and stackable as one result."""

    def _delay(self, sensor):
        so = self.solver
        t = (np.arange(0, sensor.ngate * so.oversampling_time) / so.oversampling_time - sensor.nominal_gate) / sensor.pulse_bandwidth
        # (the reference coarsens its coordinates with the data: the delay of a gate is the mean over its sub-gates)
        return t if so.return_oversampled else t.reshape(-1, so.oversampling_time).mean(axis=1)

    def _doppler(self, sensor):
        so = self.solver
        half = sensor.ndoppler // 2 * so.oversampling_doppler
        f = np.arange(-half + 0.5, +half) * (sensor.pulse_repetition_frequency / (so.oversampling_doppler * sensor.ndoppler))
        if so.return_oversampled or so.oversampling_doppler == 1:
            return f
        return f.reshape(-1, so.oversampling_doppler).mean(axis=1)

    def _names(self, n_boundaries):
        return self.solver.contributions(n_boundaries)[0]

    def _coords(self, sensor, n_boundaries):
        coords = [("delay", self._delay(sensor)), ("doppler_frequency", self._doppler(sensor)), ("theta_inc", [0]), ("theta", [0])]
        names = self._names(n_boundaries)
        return ([("contribution", names)] if names else []) + coords

    def _values(self, values, n_boundaries):
        """[..., rows, n_t, n_d] -> [..., n_t, n_d, 1, 1], or [..., n_rows, n_t, n_d, 1, 1] (the total is the last row)."""
        n_rows = len(self._names(n_boundaries))
        values = values[..., :n_rows, :, :] if self.solver.return_contributions != "no" else values[..., 0, :, :]
        return values[..., None, None]

    def _n_boundaries(self, out, slot):
        return out.n_boundaries[slot]

    def _stackable(self, n_boundaries):
        """One contribution per interface: snowpacks of different depths do not share the coordinate."""
        return self.solver.return_contributions != "full" or len(set(n_boundaries.tolist())) == 1

    @staticmethod
    def _attrs(sensor):
        return dict(pulse_bandwidth=float(sensor.pulse_bandwidth), nominal_gate=float(sensor.nominal_gate),
                    pulse_repetition_frequency=float(sensor.pulse_repetition_frequency), ndoppler=float(sensor.ndoppler))

    def _z_coord(self, sensor, foreign=False):
        """z_gate lies on the delay of the data; the reference counts its delay from the first gate."""
        return ("delay", self._delay(sensor) + (sensor.nominal_gate / sensor.pulse_bandwidth if foreign else 0.0))

    def _foreign_coords(self, sensor):
        return dict(_LrmSolution._foreign_coords(self, sensor),
                    doppler_bin=("doppler_frequency", self._doppler(sensor) / sensor.pulse_repetition_frequency * sensor.ndoppler))
