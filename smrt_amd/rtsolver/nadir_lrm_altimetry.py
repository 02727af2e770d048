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

from .._native import PackedLrmParams
from ..core.error import SMRTError
from ..core.globalconstants import C_SPEED
from ..core.result import AltimetryResult, LabeledArray
from ..core.sensor import Altimeter
from ..interface.flat import Flat
from ..interface.fresnel import reflection_diagonal
from ..interface.transparent import Transparent
from .dort import get_context
from .iterative_first_order import IterativeFirstOrder, _Packer
from .lrm_waveform_model import Brown1977  # noqa: F401  (waveform_model=Brown1977)
from .solver_base import (LayeredSolution, SolverBase, carry_plan_facts, check_error_handling, coherent_factor, layer_permittivities,
                          positive_integer)

CONTRIBUTIONS = ["surface", "interfaces", "volume", "total"]


class NadirLRMAltimetry(SolverBase):
    """Options as smrt/rtsolver/nadir_lrm_altimetry.py; `devices` (list of GPU indices; the first is used) is smrt_amd's own."""

    _broadcast_capability = {}
    NAME = "nadir_lrm_altimetry"
    ATMOSPHERE = "the {} solver can not handle atmosphere."
    CHECKS_SENSOR_FIRST = False

    def __init__(self, waveform_model=None, oversampling_time=10, return_oversampled=False, skip_pfs_convolution=False,
                 return_contributions=False, compute_coherent_reflection=True, theta_inc_sampling=8, error_handling="exception",
                 devices=None):
        check_error_handling(error_handling)
        if waveform_model is not None and getattr(waveform_model, "__name__", "") not in ("Brown1977", "brown_1977"):
            raise SMRTError("the nadir_lrm_altimetry solver offers the Brown1977 waveform model only (a model without an "
                            "analytical PFS cannot run in the reference either)")
        self.oversampling = positive_integer(oversampling_time, "oversampling_time")
        self.theta_inc_sampling = positive_integer(theta_inc_sampling, "theta_inc_sampling")
        if skip_pfs_convolution and theta_inc_sampling > 1:
            raise SMRTError("skip_pfs_convolution is offered with theta_inc_sampling=1 only (the reference returns an array "
                            "that does not fit its coordinates otherwise)")
        self.error_handling = error_handling
        self.return_oversampled, self.skip_pfs_convolution = bool(return_oversampled), bool(skip_pfs_convolution)
        self.return_contributions = bool(return_contributions)
        self.compute_coherent_reflection = bool(compute_coherent_reflection)
        self.devices = devices

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
        self._refuse_atmosphere(sp)
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
    @staticmethod
    def _sensor_key(sensor):
        return tuple(float(getattr(sensor, a)) for a in ("altitude", "pulse_bandwidth", "beamwidth_alongtrack", "beamwidth_acrosstrack",
                                                         "antenna_gain", "ngate", "nominal_gate", "pitch_angle", "roll_angle"))

    def _snowpack_key(self, sp, on_host):
        return sp, on_host    # (checked per group: what is refused depends on the sensor)

    def _context(self):
        return get_context((self.devices or [None])[0])   # (this module's name: the CPU tests put a stand-in here)

    def _solution(self, sensors, packs, sens_idx, pack_idx):
        return _Solution(self, sensors, packs, sens_idx, pack_idx)

    def _prepare_group(self, ctx, g):
        surf = np.array([self._check_snowpack(sp, g.sensor0) for sp in g.sps])
        g.packer.host_emmodels = None
        bare = [sp if sp.substrate is None else _without_substrate(sp, g.packer) for sp in g.sps]
        g.batch = g.packer._pack(g.sensor0, bare, g.u_freq, g.names, g.sensor_of)
        t_inc = self._t_inc(g.sensor0)
        options = dict(oversampling=self.oversampling, t_inc=t_inc, return_contributions=self.return_contributions,
                       return_oversampled=self.return_oversampled, skip_pfs_convolution=self.skip_pfs_convolution,
                       sigma_surface=surf[:, 0] if surf[:, 0].any() else None, surface_slope=surf[:, 1] if surf[:, 1].any() else None)
        itf = self._interface_values(ctx, g.batch, g.packer, g.sensor0, g.sps, g.u_freq, t_inc, options)
        g.params = PackedLrmParams(g.sensor0, interface_values=itf, **options)

    def _launch(self, ctx, g):
        return ctx.lrm_run(g.batch, g.params, pairs=g.pairs)

    # ---- what the host evaluates (include/smrt_dort.h: smrt_lrm_params.interface_values) ----------------------------
    def _interface_values(self, ctx, batch, packer, sensor0, sps, freqs, t_inc, options):
        """[F, S, Lmax + 1, 1 + n_mu] or None when every interface is Flat and there is no substrate: the one-way transmission at
        nadir (NaN: Flat, -1: Transparent, both on the device) and the echo per incidence sample of every boundary."""
        def on_device(itf):
            return isinstance(itf, (Flat, Transparent))

        if all(on_device(i) for sp in sps for i in sp.interfaces) and all(sp.substrate is None for sp in sps):
            return None
        F, S, Lmax, n_mu = len(freqs), len(sps), int(batch.struct.n_layers_max), len(t_inc)
        params = None if packer.host_emmodels is not None else PackedLrmParams(sensor0, **dict(options, sigma_surface=None, surface_slope=None))
        eps = layer_permittivities(ctx, batch, packer, params)[..., 0].reshape(F, S, Lmax)   # (the real part: DESIGN.md 4h)
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
            echo = echo + specular * coherent_factor(sensor, wavenumber, obj.roughness_rms, mu)
        return echo


def _without_substrate(sp, packer):
    """The snowpack as DORT's packer sees it here: the substrate enters through the interface values, not through the batch."""
    from ..core.snowpack import Snowpack

    bare = Snowpack(layers=sp.layers, interfaces=[Flat() for _ in sp.layers])
    carry_plan_facts(packer, sp, bare)
    return bare


class _Solution(LayeredSolution):
    """Outputs of the device batches of one call, addressable per simulation and stackable as one result.  The SAR solver's
    (rtsolver/nadir_sar_altimetry.py) differs in the coordinates alone: what it replaces is marked."""

    LAYER_EXTRA = ("backward_scattering",)

    def _delay(self, sensor):
        so = self.solver
        t_gate = np.arange(0, sensor.ngate * so.oversampling) / (sensor.pulse_bandwidth * so.oversampling)
        if so.oversampling > 1 and not so.return_oversampled:
            t_gate = t_gate[::so.oversampling]
        return t_gate - sensor.nominal_gate / sensor.pulse_bandwidth

    def _coords(self, sensor, n_boundaries=None):   # (replaced)
        coords = [("delay", self._delay(sensor)), ("theta_inc", [0]), ("theta", [0])]
        return ([("contribution", CONTRIBUTIONS)] if self.solver.return_contributions else []) + coords

    def _values(self, values, n_boundaries=None):   # (replaced)
        """[..., rows, n] -> [..., n, 1, 1], or [..., 4, n, 1, 1] with the total last."""
        if self.solver.return_contributions:
            values = np.concatenate([values, np.sum(values, axis=-2)[..., None, :]], axis=-2)
        else:
            values = values[..., 0, :]
        return values[..., None, None]

    def _n_boundaries(self, out, slot):   # (replaced: the SAR solver's contributions depend on the boundaries of the snowpack)
        return None

    def _stackable(self, n_boundaries):   # (replaced)
        return True

    def _z_coord(self, sensor, foreign=False):   # (replaced)
        return ("delay", self._delay(sensor))

    def _foreign_coords(self, sensor):   # (extended)
        return dict(gate=("delay", self._delay(sensor) * sensor.pulse_bandwidth + sensor.nominal_gate))

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
        sensor, group = self.sensors[self.sens_idx[i]], self.group_of[i]
        out, row = self.outputs[group], self.row_of[i]
        nb = self._n_boundaries(out, self._slot(group, self.pack_idx[i]))
        other, _ = self._other(i)   # (the layers as solved: the SAR solver prunes)
        coords = self._coords(sensor, nb)
        values = self._values(out.values[row], nb)
        foreign = self._foreign(sensor)
        if foreign is not None:   # as the reference builds it: the gate as a coordinate of delay where xarray can, z_gate an attribute
            cls, labelled = foreign
            data = labelled(values, coords)
            if hasattr(data, "assign_coords"):
                data = data.assign_coords(**self._foreign_coords(sensor))
            res = cls(data, channel_map=sensor.channel_map,
                      other_data={k: labelled(v.values, list(v.coords.items()), name=v.name) for k, v in other.items()})
            res.z_gate = labelled(out.z_gate[row].copy(), [self._z_coord(sensor, foreign=True)], name="z_gate")
            return res
        z_gate = LabeledArray(out.z_gate[row].copy(), [self._z_coord(sensor)], name="z_gate")
        return self._result(sensor, LabeledArray(values, coords), z_gate, other)

    def stacked_result(self, plan):
        grid = self._grid(plan)
        if grid is None or self._foreign(grid[0]) is not None:
            return None
        sensor0, lead, shape = grid
        out, order = self.outputs[0], self.row_of
        nbs = self._n_boundaries(out, self._slot(0, self.pack_idx))
        if not self._stackable(nbs):
            return None
        nb = None if nbs is None else int(nbs[0])
        values = self._values(out.values[order], nb)
        data = LabeledArray(values.reshape(shape + values.shape[1:]), lead + self._coords(sensor0, nb))
        z_gate = LabeledArray(out.z_gate[order].reshape(shape + (-1,)), lead + [self._z_coord(sensor0)], name="z_gate")
        return self._result(sensor0, data, z_gate, self._stacked_layers(lead, shape)[0])
